"""CPU: the filtered-search extension's surface -- ArrowSpace.subset / search_subset / score_items and ItemSubset (also under
the reference module name) and the C ABI symbols behind them.  No compute call: the GPU behaviour is tests/test_gpu_subset.py's."""
import ctypes
import inspect
import os

import numpy as np
import pytest

SYMBOLS = ("as_subset_create", "as_subset_size", "as_subset_ids", "as_subset_free", "as_search_subset", "as_score_items")


@pytest.fixture(scope="module")
def asp():
    import __graft_entry__ as g
    g.build()
    import pyarrowspace_amd
    return pyarrowspace_amd


def test_methods_and_itemsubset_exist_under_both_module_names(asp):
    import arrowspace
    for mod in (asp, arrowspace):
        for name in ("subset", "search_subset", "score_items"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
        assert inspect.isclass(mod.ItemSubset)
    assert arrowspace.ItemSubset is asp.ItemSubset and "ItemSubset" in asp.__all__
    assert list(inspect.signature(asp.ArrowSpace.subset).parameters) == ["self", "ids_or_mask"]
    assert list(inspect.signature(asp.ArrowSpace.search_subset).parameters) == ["self", "item", "gl", "tau", "subset"]
    assert list(inspect.signature(asp.ArrowSpace.score_items).parameters) == ["self", "item", "gl", "tau", "ids"]
    assert asp.ItemSubset.__doc__.startswith("Extension:")
    assert isinstance(asp.ItemSubset.size, property) and callable(asp.ItemSubset.ids)
    with pytest.raises(ValueError, match="cannot be constructed directly"):
        asp.ItemSubset()


def test_library_exports_the_subset_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert "typedef struct as_subset as_subset;" in hdr


def test_null_arguments_are_rejected_without_a_gpu(asp):
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    out = ctypes.c_void_p()
    ids = (ctypes.c_int64 * 2)(0, 1)
    assert L.as_subset_create(None, ids, 2, ctypes.byref(out)) == EINVAL and not out.value
    assert L.as_subset_create(None, None, 0, None) == EINVAL
    ln, lq = ctypes.c_int64(0), ctypes.c_double(0.0)
    assert L.as_search_subset(None, None, None, 0, 0.5, None, None, None, ctypes.byref(ln), ctypes.byref(lq)) == EINVAL
    assert L.as_score_items(None, None, None, 0, 0.5, None, 0, None, ctypes.byref(lq)) == EINVAL
    assert L.as_subset_ids(None, None) == EINVAL
    assert "null argument" in asp._lib.last_error()
    assert L.as_subset_size(None) == 0
    assert L.as_subset_free(None) is None
    assert L.as_subset_set_timing(None, 1) is None
    assert L.as_subset_kernel_us(None) == 0.0


def test_ids_are_typed_before_any_device_work(asp):
    f = asp._item_ids
    assert f([3, 1, 1], 5).tolist() == [3, 1, 1] and f([3, 1, 1], 5).dtype == "int64"
    assert f([], 5).shape == (0,) and f(np.array([]), 5).dtype == "int64" and f((), 5).shape == (0,)
    assert f([True, False, True, False, True], 5).tolist() == [0, 2, 4]
    with pytest.raises(TypeError):
        f([1.0, 2.0], 5)
    with pytest.raises(TypeError):
        f([[1, 2]], 5)
    with pytest.raises(ValueError):
        f([True, False], 5)
