"""CPU: the surface of the per-query candidate lists -- ArrowSpace.search_batch_lists / score_lists_batch / lists_counters (also
under the reference module name), the C ABI symbols behind them and the `_id_lists` helper.  No compute call: the GPU behaviour
is tests/test_gpu_lists.py's."""
import ctypes
import inspect
import os

import numpy as np
import pytest

SYMBOLS = ("as_score_lists_batch", "as_search_lists_batch", "as_lists_counters", "as_lists_kernel_us")


@pytest.fixture(scope="module")
def asp():
    import __graft_entry__ as g
    g.build()
    import pyarrowspace_amd
    return pyarrowspace_amd


def test_methods_exist_under_both_module_names(asp):
    import arrowspace
    for mod in (asp, arrowspace):
        for name in ("search_batch_lists", "score_lists_batch", "lists_counters"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
    assert arrowspace.ArrowSpace is asp.ArrowSpace
    for name in ("search_batch_lists", "score_lists_batch"):
        assert list(inspect.signature(getattr(asp.ArrowSpace, name)).parameters) == ["self", "items", "gl", "tau", "lists"]
    assert list(inspect.signature(asp.ArrowSpace.lists_counters).parameters) == ["self"]


def test_library_exports_the_lists_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert '"lists_timing"' in hdr


def test_null_arguments_are_rejected_without_a_gpu(asp):
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    ln = (ctypes.c_int64 * 2)(7, 7)
    lq = (ctypes.c_double * 2)(3.0, 3.0)
    st = (ctypes.c_int32 * 2)(9, 9)
    q = (ctypes.c_double * 8)()
    ids = (ctypes.c_int64 * 2)(0, 1)
    offs = (ctypes.c_int64 * 3)(0, 1, 2)
    sc = (ctypes.c_double * 2)(5.0, 5.0)
    assert L.as_search_lists_batch(None, None, q, 2, 4, 0.5, ids, offs, None, None, ln, lq, st) == EINVAL
    assert "as_search_lists_batch: null argument" in asp._lib.last_error()
    assert list(ln) == [7, 7] and list(lq) == [3.0, 3.0] and list(st) == [9, 9]   # nothing was written
    assert L.as_search_lists_batch(None, None, None, 0, 4, 0.5, None, None, None, None, None, None, None) == EINVAL
    assert L.as_score_lists_batch(None, None, q, 2, 4, 0.5, ids, offs, sc, lq, st) == EINVAL
    assert "as_score_lists_batch: null argument" in asp._lib.last_error()
    assert list(sc) == [5.0, 5.0] and list(lq) == [3.0, 3.0] and list(st) == [9, 9]
    assert L.as_score_lists_batch(None, None, None, 0, 4, 0.5, None, None, None, None, None) == EINVAL
    out = (ctypes.c_int64 * 4)(1, 2, 3, 4)
    assert L.as_lists_counters(None, out, 4) == EINVAL and list(out) == [1, 2, 3, 4]
    assert L.as_lists_kernel_us(None) == 0.0


def test_the_timing_switch_is_a_tuning_key(asp):
    try:
        assert asp._L.as_set_tuning(b"lists_timing", 1) == 0
    finally:
        assert asp._L.as_set_tuning(b"lists_timing", 0) == 0
    assert asp._L.as_set_tuning(b"list_timing", 1) == 1   # an unknown key


def test_id_lists_from_sequences(asp):
    ids, offs = asp._id_lists([[3, 1, 1], [], np.array([7, 0]), (5,)], 10)
    assert ids.dtype == np.int64 and offs.dtype == np.int64 and ids.flags.c_contiguous
    assert ids.tolist() == [3, 1, 1, 7, 0, 5] and offs.tolist() == [0, 3, 3, 5, 6]
    ids, offs = asp._id_lists([], 10)
    assert ids.tolist() == [] and offs.tolist() == [0] and ids.dtype == np.int64
    ids, offs = asp._id_lists([[], []], 10)
    assert ids.tolist() == [] and offs.tolist() == [0, 0, 0]


def test_id_lists_from_a_2d_array(asp):
    a = np.array([[4, 2, 9], [0, 0, 1]], dtype=np.int32)
    ids, offs = asp._id_lists(a, 10)
    assert ids.dtype == np.int64 and ids.tolist() == [4, 2, 9, 0, 0, 1] and offs.tolist() == [0, 3, 6]
    ids, offs = asp._id_lists(np.empty((3, 0), dtype=np.int64), 10)
    assert ids.tolist() == [] and offs.tolist() == [0, 0, 0, 0]


def test_id_lists_from_boolean_masks(asp):
    m0 = np.zeros(6, dtype=bool)
    m0[[1, 4]] = True
    m1 = np.ones(6, dtype=bool)
    for masks in ([m0, m1, np.zeros(6, dtype=bool)], np.stack([m0, m1, np.zeros(6, dtype=bool)])):
        ids, offs = asp._id_lists(masks, 6)
        assert ids.tolist() == [1, 4, 0, 1, 2, 3, 4, 5] and offs.tolist() == [0, 2, 8, 8]
    with pytest.raises(ValueError):
        asp._id_lists([np.ones(5, dtype=bool)], 6)   # a mask of the wrong length


def test_id_lists_refuse_float_ids(asp):
    with pytest.raises(TypeError):
        asp._id_lists([[1, 2], [1.5]], 10)
    with pytest.raises(TypeError):
        asp._id_lists(np.array([[1.0, 2.0]]), 10)
    with pytest.raises(TypeError):
        asp._id_lists([np.array([1.0])], 10)
