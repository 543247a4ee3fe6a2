"""CPU: the batched filtered-search extension's surface -- ArrowSpace.search_batch_subset / score_items_batch (also under the
reference module name) and the C ABI symbols behind them.  No compute call: the GPU behaviour is tests/test_gpu_subset_batch.py's."""
import ctypes
import inspect
import os

import pytest

SYMBOLS = ("as_search_subset_batch", "as_score_items_batch")


@pytest.fixture(scope="module")
def asp():
    import __graft_entry__ as g
    g.build()
    import pyarrowspace_amd
    return pyarrowspace_amd


def test_methods_exist_under_both_module_names(asp):
    import arrowspace
    for mod in (asp, arrowspace):
        for name in ("search_batch_subset", "score_items_batch"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
    assert arrowspace.ArrowSpace is asp.ArrowSpace
    assert list(inspect.signature(asp.ArrowSpace.search_batch_subset).parameters) == ["self", "items", "gl", "tau", "subset"]
    assert list(inspect.signature(asp.ArrowSpace.score_items_batch).parameters) == ["self", "items", "gl", "tau", "ids"]


def test_library_exports_the_batched_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert '"subset_batch_mib"' in hdr


def test_null_arguments_are_rejected_without_a_gpu(asp):
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    ln = (ctypes.c_int64 * 2)(7, 7)
    lq = (ctypes.c_double * 2)()
    st = (ctypes.c_int32 * 2)()
    q = (ctypes.c_double * 8)()
    ids = (ctypes.c_int64 * 2)(0, 1)
    assert L.as_search_subset_batch(None, None, q, 2, 4, 0.5, None, None, None, ln, lq, st) == EINVAL
    assert "as_search_subset_batch: null argument" in asp._lib.last_error()
    assert list(ln) == [7, 7]   # nothing was written
    assert L.as_search_subset_batch(None, None, None, 0, 4, 0.5, None, None, None, None, None, None) == EINVAL
    assert L.as_score_items_batch(None, None, q, 2, 4, 0.5, ids, 2, None, lq, st) == EINVAL
    assert "as_score_items_batch: null argument" in asp._lib.last_error()
    assert L.as_score_items_batch(None, None, None, 0, 4, 0.5, None, 0, None, None, None) == EINVAL


def test_the_chunk_budget_is_a_tuning_key(asp):
    try:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 1) == 0
    finally:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 256) == 0
    assert asp._L.as_set_tuning(b"subset_batch_mb", 1) == 1   # an unknown key
