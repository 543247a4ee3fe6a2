"""CPU: the surface of fused multi-query search -- ArrowSpace.search_fused / score_fused / fused_counters (also under the reference
module name), the C ABI symbols behind them, the argument checks the Python layer makes before it enters the library, and the
numpy reference tests/fused_ref.py against a plain Python-float loop.  No compute call: the GPU behaviour is
tests/test_gpu_fused.py's."""
import ctypes
import inspect
import math
import os
import struct

import numpy as np
import pytest

import fused_ref

SYMBOLS = ("as_search_fused", "as_score_fused", "as_fused_counters", "as_fused_kernel_us")


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
        for name in ("search_fused", "score_fused", "fused_counters"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
    sig = inspect.signature(asp.ArrowSpace.search_fused)
    assert list(sig.parameters) == ["self", "items", "gl", "tau", "weights", "mode", "subset", "on_zero_lambda"]
    assert [sig.parameters[p].default for p in ("weights", "mode", "subset", "on_zero_lambda")] == [None, "sum", None, "raise"]
    sig = inspect.signature(asp.ArrowSpace.score_fused)
    assert list(sig.parameters) == ["self", "items", "gl", "tau", "ids", "weights", "mode", "on_zero_lambda"]
    assert [sig.parameters[p].default for p in ("weights", "mode", "on_zero_lambda")] == [None, "sum", "raise"]


def test_library_exports_the_fused_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert '"fused_timing"' in hdr


def test_null_arguments_are_rejected_without_a_gpu(asp):
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    q = (ctypes.c_double * 8)()
    idx = (ctypes.c_int64 * 2)(7, 7)
    sc = (ctypes.c_double * 2)(5.0, 5.0)
    ln = ctypes.c_int64(9)
    lq = (ctypes.c_double * 2)(3.0, 3.0)
    st = (ctypes.c_int32 * 2)(9, 9)
    assert L.as_search_fused(None, None, q, 2, 4, 0.5, None, 0, 0, None, idx, sc, ctypes.byref(ln), lq, st) == EINVAL
    assert "as_search_fused: null argument" in asp._lib.last_error()
    assert list(idx) == [7, 7] and list(sc) == [5.0, 5.0] and ln.value == 9 and list(lq) == [3.0, 3.0] and list(st) == [9, 9]
    ids = (ctypes.c_int64 * 2)(0, 1)
    assert L.as_score_fused(None, None, q, 2, 4, 0.5, None, 1, 1, ids, 2, sc, lq, st) == EINVAL
    assert "as_score_fused: null argument" in asp._lib.last_error()
    assert list(sc) == [5.0, 5.0] and list(lq) == [3.0, 3.0] and list(st) == [9, 9]
    out = (ctypes.c_int64 * 4)(1, 2, 3, 4)
    assert L.as_fused_counters(None, out, 4) == EINVAL and list(out) == [1, 2, 3, 4]
    assert "as_fused_counters: null argument" in asp._lib.last_error()
    assert L.as_fused_kernel_us(None) == 0.0


def test_timing_is_a_tuning_key(asp):
    try:
        assert asp._L.as_set_tuning(b"fused_timing", 1) == 0
    finally:
        assert asp._L.as_set_tuning(b"fused_timing", 0) == 0
    assert asp._L.as_set_tuning(b"fused_timings", 1) == 1   # an unknown key


def test_argument_errors_are_raised_before_the_library_is_entered(asp):
    """A space and a graph that hold no handle are enough: every refusal comes before a handle is touched."""
    space = object.__new__(asp.ArrowSpace)
    gl = object.__new__(asp.GraphLaplacian)
    Q = np.zeros((3, 4))
    calls = (lambda **kw: space.search_fused(kw.pop("items", Q), kw.pop("gl", gl), 0.62, **kw),
             lambda **kw: space.score_fused(kw.pop("items", Q), kw.pop("gl", gl), 0.62, [0, 1], **kw))
    for call in calls:
        with pytest.raises(TypeError, match="GraphLaplacian"):
            call(gl=None)
        with pytest.raises(TypeError, match="2-D"):
            call(items=np.zeros(4))
        with pytest.raises(TypeError, match="2-D"):
            call(items=np.zeros((2, 2, 2)))
        with pytest.raises(ValueError, match="at least one"):
            call(items=np.zeros((0, 4)))
        for mode in ("mean", "SUM", "", None, 0):
            with pytest.raises(ValueError, match="mode"):
                call(mode=mode)
        for ozl in ("ignore", "", None, True):
            with pytest.raises(ValueError, match="on_zero_lambda"):
                call(on_zero_lambda=ozl)
        for w in ([1.0, 2.0], [1.0, 2.0, 3.0, 4.0], [], [[1.0, 2.0, 3.0]], 1.0):
            with pytest.raises(ValueError, match="weights"):
                call(weights=w)
        for w in ([1.0, float("nan"), 1.0], [float("inf"), 0.0, 0.0], np.array([0.0, 0.0, -np.inf])):
            with pytest.raises(ValueError, match="finite"):
                call(weights=w)
        for w in (["a", "b", "c"], [None, None, None], "abc"):
            with pytest.raises(TypeError, match="weights"):
                call(weights=w)
    Qo, w, mode, skip = asp._fused_args(Q[:, ::-1], gl, (1, -2, np.float32(0.5)), "max", "skip")
    assert Qo.flags.c_contiguous and Qo.dtype == np.float64 and w.dtype == np.float64 and w.tolist() == [1.0, -2.0, 0.5]
    assert (mode, skip) == (1, 1)
    assert asp._fused_args(Q, gl, None, "sum", "raise")[1:] == (None, 0, 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def plain_fuse(S, w, mode, served=None):
    """S13 in Python floats (IEEE doubles, one rounding per operation), one position at a time."""
    out = []
    for i in range(len(S[0])):
        F = None
        for j in range(len(S)):
            if served is not None and not served[j]:
                continue
            t = float(w[j]) * float(S[j][i])
            if F is None:
                F = t
            elif mode == "sum":
                F = F + t
            elif t > F or math.isnan(F):
                F = t
        out.append(F)
    return out


NAN = float("nan")


def test_the_reference_agrees_with_a_plain_loop_on_random_scores():
    rng = np.random.default_rng(5)
    for J, M in ((1, 7), (2, 5), (5, 33), (9, 4)):
        S = rng.standard_normal((J, M)) * 10.0 ** rng.integers(-3, 4, (J, M))
        w = rng.uniform(-1.0, 1.0, J)
        for mode in ("sum", "max"):
            assert bits(fused_ref.fuse(S, w, mode)) == bits(plain_fuse(S.tolist(), w.tolist(), mode))


def test_max_never_lets_a_nan_displace_a_number_and_the_first_largest_wins():
    S = np.array([[NAN, 1.0, NAN, 2.0, -0.0, 3.0],
                  [1.0, NAN, NAN, 2.0, 0.0, NAN],
                  [0.5, 0.5, NAN, 1.0, -0.0, 4.0]])
    w = np.array([1.0, 1.0, 2.0])
    F = fused_ref.fuse(S, w, "max")
    assert bits(F) == bits(plain_fuse(S.tolist(), w.tolist(), "max"))
    assert F[0] == 1.0 and F[1] == 1.0 and math.isnan(F[2]) and F[3] == 2.0 and F[5] == 8.0
    assert struct.pack("<d", F[4]) == struct.pack("<d", -0.0)   # 0.0 > -0.0 is false: the first of equal terms stays
    # a negative weight turns the order round
    F = fused_ref.fuse(S[:, 3:4], np.array([-1.0, -0.5, -3.0]), "max")
    assert F.tolist() == [-1.0]
    # under sum a NaN term poisons the position
    assert np.isnan(fused_ref.fuse(S, w, "sum")[:3]).all()


def test_a_skipped_row_is_left_out_with_its_weight():
    rng = np.random.default_rng(6)
    S = rng.standard_normal((4, 9))
    w = np.array([0.5, -2.0, 0.25, 1.5])
    for mode in ("sum", "max"):
        for served in ([True, False, True, True], [False, True, True, False], [False, False, False, True]):
            got = fused_ref.fuse(S, w, mode, served)
            keep = np.flatnonzero(served)
            assert bits(got) == bits(fused_ref.fuse(S[keep], w[keep], mode))
            assert bits(got) == bits(plain_fuse(S.tolist(), w.tolist(), mode, served))
        with pytest.raises(ValueError, match="served"):
            fused_ref.fuse(S, w, mode, [False] * 4)
    # a skipped first row: the next served row initialises, there is no 0 + t start (-0.0 survives)
    Z = np.array([[1.0], [-0.0]])
    assert bits(fused_ref.fuse(Z, np.array([1.0, 1.0]), "sum", [False, True])) == bits([-0.0])


def test_plus_and_minus_one_cancel_to_positive_zero():
    rng = np.random.default_rng(7)
    s = rng.standard_normal(50)
    s[:3] = (0.0, -0.0, 1e-310)
    F = fused_ref.fuse(np.stack([s, s]), np.array([1.0, -1.0]), "sum")
    assert bits(F) == bits(np.zeros(50)) == bits(plain_fuse([s.tolist(), s.tolist()], [1.0, -1.0], "sum"))
    ids = np.arange(100, 150)
    i, v = fused_ref.top(ids, F, 6)
    assert i.tolist() == [100, 101, 102, 103, 104, 105] and bits(v) == bits(np.zeros(6))


def test_top_orders_by_score_then_id_and_cuts_at_k():
    ids = np.array([9, 4, 7, 1, 3])
    F = np.array([0.5, 2.0, 0.5, -1.0, 2.0])
    i, v = fused_ref.top(ids, F, 4)
    assert i.tolist() == [3, 4, 7, 9] and v.tolist() == [2.0, 2.0, 0.5, 0.5]
    i, v = fused_ref.top(ids, F, 10)
    assert i.tolist() == [3, 4, 7, 9, 1]
    i, v = fused_ref.top(np.array([2, 1]), np.array([0.0, -0.0]), 2)   # +0.0 and -0.0 tie
    assert i.tolist() == [1, 2]
