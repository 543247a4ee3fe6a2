"""CPU: the surface of the tau sweeps over per-query candidate lists -- ArrowSpace.search_batch_lists_taus /
score_lists_batch_taus / lists_sweep_counters (also under the reference module name) and the C ABI symbols behind them.  No
compute call: the GPU behaviour is tests/test_gpu_lists_sweep.py's."""
import ctypes
import inspect
import os

import numpy as np
import pytest

SYMBOLS = ("as_score_lists_batch_taus", "as_search_lists_batch_taus", "as_lists_sweep_counters")


@pytest.fixture(scope="module")
def asp():
    import __graft_entry__ as g
    g.build()
    import pyarrowspace_amd
    return pyarrowspace_amd


def test_methods_exist_under_both_module_names(asp):
    import arrowspace
    for mod in (asp, arrowspace):
        for name in ("search_batch_lists_taus", "score_lists_batch_taus", "lists_sweep_counters"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
    assert arrowspace.ArrowSpace is asp.ArrowSpace
    for name in ("search_batch_lists_taus", "score_lists_batch_taus"):
        assert list(inspect.signature(getattr(asp.ArrowSpace, name)).parameters) == ["self", "items", "gl", "taus", "lists"]
    assert list(inspect.signature(asp.ArrowSpace.lists_sweep_counters).parameters) == ["self"]


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
    lq = (ctypes.c_double * 2)(3.0, 3.0)
    st = (ctypes.c_int32 * 2)(9, 9)
    q = (ctypes.c_double * 8)()
    taus = (ctypes.c_double * 2)(1.0, 0.62)
    ids = (ctypes.c_int64 * 2)(0, 1)
    offs = (ctypes.c_int64 * 3)(0, 1, 2)
    sc = (ctypes.c_double * 4)(5.0, 5.0, 5.0, 5.0)
    idx = (ctypes.c_int64 * 4)(8, 8, 8, 8)

    def untouched():
        return (list(ln) == [7] * 4 and list(lq) == [3.0, 3.0] and list(st) == [9, 9] and list(sc) == [5.0] * 4 and list(idx) == [8] * 4)

    assert L.as_search_lists_batch_taus(None, None, q, 2, 4, taus, 2, ids, offs, idx, sc, ln, lq, st) == EINVAL
    assert "as_search_lists_batch_taus: null argument" in asp._lib.last_error()
    assert untouched()
    assert L.as_search_lists_batch_taus(None, None, None, 0, 4, None, 0, None, None, None, None, None, None, None) == EINVAL
    assert L.as_score_lists_batch_taus(None, None, q, 2, 4, taus, 2, ids, offs, sc, lq, st) == EINVAL
    assert "as_score_lists_batch_taus: null argument" in asp._lib.last_error()
    assert untouched()
    assert L.as_score_lists_batch_taus(None, None, None, 0, 4, None, 0, None, None, None, None, None) == EINVAL
    out = (ctypes.c_int64 * 5)(1, 2, 3, 4, 5)
    assert L.as_lists_sweep_counters(None, out, 5) == EINVAL and list(out) == [1, 2, 3, 4, 5]
    assert "as_lists_sweep_counters: null argument" in asp._lib.last_error()


def test_taus_refuse_a_2d_argument(asp):
    assert asp.ArrowSpace._taus([1.0, 0.62]).tolist() == [1.0, 0.62]
    assert asp.ArrowSpace._taus([]).shape == (0,)
    with pytest.raises(TypeError):
        asp.ArrowSpace._taus(np.ones((2, 2)))
    with pytest.raises(TypeError):
        asp.ArrowSpace._taus([[1.0, 0.62]])
