"""CPU: the surface of the tau sweeps over a subset -- ArrowSpace.search_subset_taus / score_items_taus /
search_batch_subset_taus / score_items_batch_taus and subset_sweep_counters (also under the reference module name) and the C ABI
symbols behind them.  No compute call: the GPU behaviour is tests/test_gpu_subset_sweep.py's."""
import ctypes
import inspect
import os

import pytest

SYMBOLS = ("as_search_subset_taus", "as_score_items_taus", "as_search_subset_batch_taus", "as_score_items_batch_taus",
           "as_subset_sweep_counters")
METHODS = {"search_subset_taus": ["self", "item", "gl", "taus", "subset"], "score_items_taus": ["self", "item", "gl", "taus", "ids"],
           "search_batch_subset_taus": ["self", "items", "gl", "taus", "subset"],
           "score_items_batch_taus": ["self", "items", "gl", "taus", "ids"], "subset_sweep_counters": ["self"]}


@pytest.fixture(scope="module")
def asp():
    import __graft_entry__ as g
    g.build()
    import pyarrowspace_amd
    return pyarrowspace_amd


def test_methods_exist_under_both_module_names(asp):
    import arrowspace
    assert arrowspace.ArrowSpace is asp.ArrowSpace
    for mod in (asp, arrowspace):
        for name, params in METHODS.items():
            f = getattr(mod.ArrowSpace, name, None)
            assert callable(f), name
            assert f.__doc__.startswith("Extension:"), name
            assert list(inspect.signature(f).parameters) == params, name


def test_library_exports_the_sweep_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name


def test_null_arguments_are_rejected_without_a_gpu(asp):
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    ln = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    lq = (ctypes.c_double * 2)(-1.0, -1.0)
    st = (ctypes.c_int32 * 2)(-7, -7)
    q = (ctypes.c_double * 8)()
    taus = (ctypes.c_double * 2)(1.0, 0.5)
    ids = (ctypes.c_int64 * 2)(0, 1)
    out = (ctypes.c_double * 8)(*([-5.0] * 8))
    cnt = (ctypes.c_int64 * 4)(9, 9, 9, 9)

    def untouched():
        return list(ln) == [7] * 4 and list(lq) == [-1.0] * 2 and list(st) == [-7] * 2 and list(out) == [-5.0] * 8

    assert L.as_search_subset_taus(None, None, q, 4, taus, 2, None, None, None, ln, lq) == EINVAL
    assert "as_search_subset_taus: null argument" in asp._lib.last_error()
    assert untouched()
    assert L.as_search_subset_taus(None, None, None, 4, None, 0, None, None, None, None, None) == EINVAL
    assert L.as_score_items_taus(None, None, q, 4, taus, 2, ids, 2, out, lq) == EINVAL
    assert "as_score_items_taus: null argument" in asp._lib.last_error()
    assert untouched()
    assert L.as_score_items_taus(None, None, None, 4, None, 0, None, 0, None, None) == EINVAL
    assert L.as_search_subset_batch_taus(None, None, q, 2, 4, taus, 2, None, None, None, ln, lq, st) == EINVAL
    assert "as_search_subset_batch_taus: null argument" in asp._lib.last_error()
    assert untouched()
    assert L.as_search_subset_batch_taus(None, None, None, 0, 4, None, 0, None, None, None, None, None, None) == EINVAL
    assert L.as_score_items_batch_taus(None, None, q, 2, 4, taus, 2, ids, 2, out, lq, st) == EINVAL
    assert "as_score_items_batch_taus: null argument" in asp._lib.last_error()
    assert untouched()
    assert L.as_score_items_batch_taus(None, None, None, 0, 4, None, 0, None, 0, None, None, None) == EINVAL
    assert L.as_subset_sweep_counters(None, cnt, 4) == EINVAL
    assert "as_subset_sweep_counters: null argument" in asp._lib.last_error()
    assert list(cnt) == [9] * 4
