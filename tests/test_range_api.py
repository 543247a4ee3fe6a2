"""CPU: the surface of range search -- ArrowSpace.search_range / count_range / search_range_batch / count_range_batch (also
under the reference module name), the C ABI symbols behind them, the as_range handle's accessors on NULL and the `_min_scores`
helper.  No compute call: the GPU behaviour is tests/test_gpu_range.py's."""
import ctypes
import inspect
import os

import numpy as np
import pytest

SYMBOLS = ("as_search_range", "as_search_range_batch", "as_range_queries", "as_range_total", "as_range_offsets", "as_range_copy",
           "as_range_free", "as_range_counters", "as_range_kernel_us")


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
        for name in ("search_range", "count_range", "search_range_batch", "count_range_batch"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
    for name in ("search_range", "count_range"):
        sig = inspect.signature(getattr(asp.ArrowSpace, name))
        assert list(sig.parameters) == ["self", "item", "gl", "tau", "min_score", "subset"]
        assert sig.parameters["subset"].default is None
    for name in ("search_range_batch", "count_range_batch"):
        sig = inspect.signature(getattr(asp.ArrowSpace, name))
        assert list(sig.parameters) == ["self", "items", "gl", "tau", "min_score", "subset"]
        assert sig.parameters["subset"].default is None


def test_library_exports_the_range_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert "typedef struct as_range as_range;" in hdr
    assert '"range_cap"' in hdr and '"range_timing"' in hdr


def test_null_arguments_are_rejected_without_a_gpu(asp):
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    q = (ctypes.c_double * 8)()
    thr = (ctypes.c_double * 2)(0.5, 0.5)
    lq = (ctypes.c_double * 2)(3.0, 3.0)
    st = (ctypes.c_int32 * 2)(9, 9)
    h = ctypes.c_void_p(12345)
    assert L.as_search_range(None, None, q, 4, 0.5, 0.5, None, 0, ctypes.byref(h), lq) == EINVAL
    assert "as_search_range: null argument" in asp._lib.last_error()
    assert h.value is None and list(lq) == [3.0, 3.0]
    assert L.as_search_range(None, None, None, 4, 0.5, 0.5, None, 1, None, None) == EINVAL
    h = ctypes.c_void_p(12345)
    assert L.as_search_range_batch(None, None, q, 2, 4, 0.5, thr, None, 0, ctypes.byref(h), lq, st) == EINVAL
    assert "as_search_range_batch: null argument" in asp._lib.last_error()
    assert h.value is None and list(lq) == [3.0, 3.0] and list(st) == [9, 9]   # nothing else was written
    assert L.as_search_range_batch(None, None, None, 0, 4, 0.5, None, None, 0, None, None, None) == EINVAL
    out = (ctypes.c_int64 * 6)(1, 2, 3, 4, 5, 6)
    assert L.as_range_counters(None, out, 6) == EINVAL and list(out) == [1, 2, 3, 4, 5, 6]
    assert "as_range_counters: null argument" in asp._lib.last_error()
    assert L.as_range_kernel_us(None) == 0.0


def test_the_handle_accessors_are_harmless_on_null(asp):
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    assert L.as_range_queries(None) == 0
    assert L.as_range_total(None) == 0
    offs = (ctypes.c_int64 * 2)(7, 7)
    assert L.as_range_offsets(None, offs) == EINVAL and list(offs) == [7, 7]
    assert "as_range_offsets: null argument" in asp._lib.last_error()
    idx = (ctypes.c_int64 * 2)(7, 7)
    sc = (ctypes.c_double * 2)(5.0, 5.0)
    assert L.as_range_copy(None, idx, sc) == EINVAL and list(idx) == [7, 7] and list(sc) == [5.0, 5.0]
    assert "as_range_copy: null argument" in asp._lib.last_error()
    L.as_range_free(None)


def test_capacity_and_timing_are_tuning_keys(asp):
    try:
        assert asp._L.as_set_tuning(b"range_cap", 4) == 0
        assert asp._L.as_set_tuning(b"range_timing", 0) == 0
        assert asp._L.as_set_tuning(b"range_timing", 1) == 0
    finally:
        assert asp._L.as_set_tuning(b"range_cap", 0) == 0
        assert asp._L.as_set_tuning(b"range_timing", 0) == 0
    assert asp._L.as_set_tuning(b"range_caps", 4) == 1   # an unknown key


def test_min_scores_broadcasts_a_scalar(asp):
    for v in (0.25, 1, np.float32(0.25), np.float64(-3.0), np.int64(2)):
        a = asp._min_scores(v, 3)
        assert a.dtype == np.float64 and a.shape == (3,) and a.flags.c_contiguous
        assert a.tolist() == [float(v)] * 3
    assert asp._min_scores(0.5, 0).shape == (0,)
    assert asp._min_scores(-np.inf, 2).tolist() == [-np.inf, -np.inf]
    assert asp._min_scores(np.inf, 1).tolist() == [np.inf]


def test_min_scores_takes_one_threshold_per_query(asp):
    a = asp._min_scores([0.1, -np.inf, np.inf, 2], 4)
    assert a.dtype == np.float64 and a.tolist() == [0.1, -np.inf, np.inf, 2.0]
    a = asp._min_scores(np.array([1, 2, 3], dtype=np.int32)[::-1], 3)
    assert a.tolist() == [3.0, 2.0, 1.0] and a.flags.c_contiguous
    assert asp._min_scores((0.5,), 1).tolist() == [0.5]
    assert asp._min_scores([], 0).shape == (0,)   # (numpy types an empty list float64)


def test_min_scores_refuses_nan_wrong_length_and_wrong_rank(asp):
    with pytest.raises(ValueError, match="NaN"):
        asp._min_scores(float("nan"), 2)
    with pytest.raises(ValueError, match="NaN"):
        asp._min_scores([0.5, float("nan")], 2)
    with pytest.raises(ValueError, match="thresholds"):
        asp._min_scores([0.5, 0.6], 3)
    with pytest.raises(ValueError, match="thresholds"):
        asp._min_scores([0.5], 0)
    with pytest.raises(ValueError, match="1-D"):
        asp._min_scores(np.zeros((2, 2)), 2)
    with pytest.raises(ValueError, match="1-D"):
        asp._min_scores([[0.5, 0.6]], 2)


def test_min_scores_refuses_what_is_not_a_number(asp):
    for bad in ("0.5", b"0.5", ["a", "b"], None, [0.5, "x"], True, [True, False], 1j):
        with pytest.raises(TypeError):
            asp._min_scores(bad, 2)
