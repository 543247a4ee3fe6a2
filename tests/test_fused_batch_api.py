"""CPU: the surface of batched fused search -- ArrowSpace.search_fused_batch / score_fused_batch /
fused_batch_counters (also under the reference module name), the C ABI symbols behind them, the refusals the C entries make
before they touch a handle, the argument checks the Python layer makes before it enters the library, and the numpy reference
tests/fused_batch_ref.py against a plain Python-float loop.  No compute call: the GPU behaviour is tests/test_gpu_fused_batch.py's."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import fused_batch_ref

SYMBOLS = ("as_search_fused_batch", "as_score_fused_batch", "as_fused_batch_counters", "as_fused_batch_kernel_us")


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
        for name in ("search_fused_batch", "score_fused_batch", "fused_batch_counters"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
    sig = inspect.signature(asp.ArrowSpace.search_fused_batch)
    assert list(sig.parameters) == ["self", "needs", "gl", "tau", "weights", "mode", "subset", "on_zero_lambda"]
    assert [sig.parameters[p].default for p in ("weights", "mode", "subset", "on_zero_lambda")] == [None, "sum", None, "raise"]
    sig = inspect.signature(asp.ArrowSpace.score_fused_batch)
    assert list(sig.parameters) == ["self", "needs", "gl", "tau", "ids", "weights", "mode", "on_zero_lambda"]
    assert [sig.parameters[p].default for p in ("weights", "mode", "on_zero_lambda")] == [None, "sum", "raise"]
    assert list(inspect.signature(asp.ArrowSpace.fused_batch_counters).parameters) == ["self"]


def test_library_exports_the_batched_fused_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert '"fused_batch_timing"' in hdr and '"fused_batch_mib"' in hdr


def test_the_tuning_keys_are_known(asp):
    try:
        assert asp._L.as_set_tuning(b"fused_batch_timing", 1) == 0
        assert asp._L.as_set_tuning(b"fused_batch_mib", 1) == 0
    finally:
        assert asp._L.as_set_tuning(b"fused_batch_timing", 0) == 0
        assert asp._L.as_set_tuning(b"fused_batch_mib", 0) == 0
    assert asp._L.as_set_tuning(b"fused_batch_timings", 1) == 1   # an unknown key
    assert asp._L.as_set_tuning(b"fused_batch_mibs", 1) == 1


def test_null_and_bad_offset_arguments_are_rejected_without_a_gpu(asp):
    """Handles that point nowhere a library could read: every refusal below comes before a handle is touched."""
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    fake = ctypes.c_void_p(8)   # never dereferenced
    q = (ctypes.c_double * 12)()
    idx = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    sc = (ctypes.c_double * 4)(5.0, 5.0, 5.0, 5.0)
    ln = (ctypes.c_int64 * 2)(9, 9)
    lq = (ctypes.c_double * 3)(3.0, 3.0, 3.0)
    st = (ctypes.c_int32 * 2)(9, 9)
    ids = (ctypes.c_int64 * 2)(0, 1)
    good = (ctypes.c_int64 * 3)(0, 1, 3)

    def untouched():
        return (list(idx) == [7] * 4 and list(sc) == [5.0] * 4 and list(ln) == [9, 9] and list(lq) == [3.0] * 3 and list(st) == [9, 9])

    def search(sp, gr, qq, offs, b, nv, out_len=ln):
        return L.as_search_fused_batch(sp, gr, qq, offs, b, nv, 4, 0.5, None, 0, 0, None, idx, sc, out_len, lq, st)

    def score(sp, gr, qq, offs, b, nv, ids_=ids, out=sc):
        return L.as_score_fused_batch(sp, gr, qq, offs, b, nv, 4, 0.5, None, 1, 1, ids_, 2, out, lq, st)

    for args in ((None, None, q, good), (None, fake, q, good), (fake, None, q, good), (fake, fake, None, good), (fake, fake, q, None)):
        assert search(*args, 2, 3) == EINVAL
        assert "as_search_fused_batch: null argument" in asp._lib.last_error() and untouched()
        assert score(*args, 2, 3) == EINVAL
        assert "as_score_fused_batch: null argument" in asp._lib.last_error() and untouched()
    assert search(fake, fake, q, good, 2, 3, out_len=None) == EINVAL and "null argument" in asp._lib.last_error() and untouched()
    assert score(fake, fake, q, good, 2, 3, ids_=None) == EINVAL and "null argument" in asp._lib.last_error() and untouched()
    assert score(fake, fake, q, good, 2, 3, out=None) == EINVAL and "null argument" in asp._lib.last_error() and untouched()
    # offsets: start at 0, increase strictly, end at nv; b >= 1
    bad = (((1, 2, 3), 2, 3, "start at 0"), ((0, 1, 2), 2, 3, "end at nv"), ((0, 1, 4), 2, 3, "end at nv"), ((0, 0, 3), 2, 3, "strictly"),
           ((0, 3, 3), 2, 3, "strictly"), ((0, 4, 3), 2, 3, "strictly"), ((0, 1, 3), 0, 0, "b must be"), ((0, 1, 3), -1, 3, "b must be"))
    for offs, b, nv, what in bad:
        o = (ctypes.c_int64 * 3)(*offs)
        assert search(fake, fake, q, o, b, nv) == EINVAL and what in asp._lib.last_error(), (offs, asp._lib.last_error())
        assert "as_search_fused_batch" in asp._lib.last_error() and untouched()
        assert score(fake, fake, q, o, b, nv) == EINVAL and what in asp._lib.last_error(), (offs, asp._lib.last_error())
        assert "as_score_fused_batch" in asp._lib.last_error() and untouched()
    out = (ctypes.c_int64 * 6)(1, 2, 3, 4, 5, 6)
    assert L.as_fused_batch_counters(None, out, 6) == EINVAL and list(out) == [1, 2, 3, 4, 5, 6]
    assert "as_fused_batch_counters: null argument" in asp._lib.last_error()
    assert L.as_fused_batch_kernel_us(None) == 0.0


def test_argument_errors_are_raised_before_the_library_is_entered(asp):
    """A space and a graph that hold no handle are enough: every refusal comes before a handle is touched."""
    space = object.__new__(asp.ArrowSpace)
    gl = object.__new__(asp.GraphLaplacian)
    N = [np.zeros((3, 4)), np.zeros((1, 4))]
    calls = (lambda **kw: space.search_fused_batch(kw.pop("needs", N), kw.pop("gl", gl), 0.62, **kw),
             lambda **kw: space.score_fused_batch(kw.pop("needs", N), kw.pop("gl", gl), 0.62, [0, 1], **kw))
    for call in calls:
        with pytest.raises(TypeError, match="GraphLaplacian"):
            call(gl=None)
        # a need that is not 2-D (the message names it), needs that are no sequence of needs
        with pytest.raises(TypeError, match="need 1 must be a 2-D"):
            call(needs=[np.zeros((2, 4)), np.zeros(4)])
        with pytest.raises(TypeError, match="need 0 must be a 2-D"):
            call(needs=[np.zeros((2, 2, 4))])
        for needs in (np.zeros((3, 4)), np.zeros(4), np.zeros((2, 2, 2, 4)), 1.0, "ab", None):
            with pytest.raises(TypeError, match="needs"):
                call(needs=needs)
        for needs in ([], np.zeros((0, 2, 4))):
            with pytest.raises(ValueError, match="at least one need"):
                call(needs=needs)
        with pytest.raises(ValueError, match="need 1 must hold at least one"):
            call(needs=[np.zeros((2, 4)), np.zeros((0, 4))])
        with pytest.raises(ValueError, match="at least one"):
            call(needs=np.zeros((2, 0, 4)))
        with pytest.raises(ValueError, match="need 2 has D = 5"):
            call(needs=[np.zeros((2, 4)), np.zeros((1, 4)), np.zeros((1, 5))])
        for mode in ("mean", "SUM", "", None, 0):
            with pytest.raises(ValueError, match="mode"):
                call(mode=mode)
        for ozl in ("ignore", "", None, True):
            with pytest.raises(ValueError, match="on_zero_lambda"):
                call(on_zero_lambda=ozl)
        # a wrong number of entries, a wrong weight count or rank inside a need
        for w in ([[1.0, 2.0, 3.0]], [[1.0, 2.0, 3.0], [1.0], [1.0]], [], 1.0, np.ones((3, 3))):
            with pytest.raises(ValueError, match="weights"):
                call(weights=w)
        for w, who in (([[1.0, 2.0], [1.0]], "need 0"), ([[1.0, 2.0, 3.0], [1.0, 2.0]], "need 1"), ([None, []], "need 1"),
                       ([[[1.0, 2.0, 3.0]], None], "need 0"), ([1.0, 1.0], "need 0")):
            with pytest.raises(ValueError, match=f"weights.*{who}"):
                call(weights=w)
        for w, who in (([[1.0, float("nan"), 1.0], [1.0]], "need 0"), ([None, [float("inf")]], "need 1"),
                       ([np.array([0.0, 0.0, -np.inf]), None], "need 0")):
            with pytest.raises(ValueError, match=f"{who}.*finite"):
                call(weights=w)
        for w, who in (([["a", "b", "c"], [1.0]], "need 0"), ([None, "a"], "need 1"), ([[1.0, 2.0, 3.0], [None]], "need 1")):
            with pytest.raises(TypeError, match=f"weights.*{who}"):
                call(weights=w)
        with pytest.raises(TypeError, match="weights"):
            call(weights="ab")
    # what reaches the library: the flattened vectors, the offsets, the flattened weights with the defaults filled in
    A, B = np.arange(12.0).reshape(3, 4)[:, ::-1], np.arange(4.0).reshape(1, 4)
    V, offs, w, mode, skip = asp._fused_batch_args([A, B], gl, [None, (np.float32(0.5),)], "max", "skip")
    assert V.flags.c_contiguous and V.dtype == np.float64 and V.tolist() == np.concatenate([A, B]).tolist()
    assert offs.dtype == np.int64 and offs.tolist() == [0, 3, 4]
    assert w.dtype == np.float64 and w.tolist() == [1.0 / 3, 1.0 / 3, 1.0 / 3, 0.5] and (mode, skip) == (1, 1)
    V, offs, w, mode, skip = asp._fused_batch_args(np.zeros((5, 2, 4)), gl, None, "sum", "raise")
    assert V.shape == (10, 4) and offs.tolist() == [0, 2, 4, 6, 8, 10] and w is None and (mode, skip) == (0, 0)
    assert asp._fused_batch_args(np.zeros((2, 2, 4)), gl, [None, None], "sum", "raise")[2] is None
    w = asp._fused_batch_args(np.zeros((2, 2, 4)), gl, np.array([[1, -2], [3, 4]]), "sum", "raise")[2]
    assert w.dtype == np.float64 and w.tolist() == [1.0, -2.0, 3.0, 4.0]
    assert asp._fused_batch_args([[[0.0, 1.0]], [[1.0, 2.0], [3.0, 4.0]]], gl, None, "sum", "raise")[1].tolist() == [0, 1, 3]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def plain_fuse_batch(S, offsets, w, mode, served=None):
    """S15's fold in Python floats (IEEE doubles, one rounding per operation), one need and one position at a time."""
    out = []
    for b in range(len(offsets) - 1):
        row = []
        for i in range(len(S[0])):
            F = None
            for j in range(offsets[b], offsets[b + 1]):
                if served is not None and not served[j]:
                    continue
                t = float(w[j]) * float(S[j][i])
                if F is None:
                    F = t
                elif mode == "sum":
                    F = F + t
                elif t > F or math.isnan(F):
                    F = t
            row.append(float("nan") if F is None else F)
        out.append(row)
    return out


NAN = float("nan")


def test_the_batch_reference_agrees_with_a_plain_loop():
    rng = np.random.default_rng(15)
    for Js, M in (((1,), 7), ((2, 1, 5), 9), ((3, 3, 3, 3), 4), ((1, 9, 2), 33)):
        offs = np.concatenate([[0], np.cumsum(Js)]).tolist()
        S = rng.standard_normal((offs[-1], M)) * 10.0 ** rng.integers(-3, 4, (offs[-1], M))
        w = rng.uniform(-1.0, 1.0, offs[-1])
        for mode in ("sum", "max"):
            F = fused_batch_ref.fuse_batch(S, offs, w, mode)
            assert F.shape == (len(Js), M) and F.dtype == np.float64
            assert bits(F) == bits(plain_fuse_batch(S.tolist(), offs, w.tolist(), mode))
    with pytest.raises(ValueError):
        fused_batch_ref.fuse_batch(np.zeros((3, 2)), [0, 1, 2], np.ones(3), "sum")   # offsets do not end at the rows
    with pytest.raises(ValueError):
        fused_batch_ref.fuse_batch(np.zeros((3, 2)), [0, 0, 3], np.ones(3), "sum")   # an empty need
    assert fused_batch_ref.default_weights([0, 1, 4, 6]).tolist() == [1.0, 1.0 / 3, 1.0 / 3, 1.0 / 3, 0.5, 0.5]


def test_negative_zero_nan_under_max_and_an_unserved_row():
    # need 0: a -0.0 term first (it survives: there is no 0 + t start) and a NaN term; need 1: NaN terms under max; need 2: one row
    S = np.array([[-0.0, 1.0, NAN, 2.0],
                  [0.0, NAN, NAN, -0.0],
                  [NAN, 1.0, NAN, 2.0],
                  [1.0, NAN, NAN, 2.0],
                  [0.5, 0.5, NAN, 1.0],
                  [-0.0, -0.0, 3.0, NAN]])
    offs = [0, 2, 5, 6]
    w = np.array([1.0, 1.0, 1.0, 1.0, 2.0, 1.0])
    for mode in ("sum", "max"):
        assert bits(fused_batch_ref.fuse_batch(S, offs, w, mode)) == bits(plain_fuse_batch(S.tolist(), offs, w.tolist(), mode))
    F = fused_batch_ref.fuse_batch(S, offs, w, "max")
    assert bits(F[0, :1]) == bits([-0.0])          # 0.0 > -0.0 is false: the first of equal terms stays
    assert F[0, 1] == 1.0 and math.isnan(F[0, 2])  # a NaN never displaces a number; all NaN stays NaN
    assert F[1].tolist()[:2] == [1.0, 1.0] and math.isnan(F[1, 2]) and F[1, 3] == 2.0
    assert bits(F[2]) == bits(S[5])
    Fs = fused_batch_ref.fuse_batch(S, offs, w, "sum")
    assert bits(Fs[0, :1]) == bits([0.0]) and bits(Fs[0, 3:]) == bits([2.0]) and np.isnan(Fs[0, 1:3]).all()   # -0.0 + 0.0 = +0.0
    # unserved rows: left out with their weight; a skipped first row: the next served row initialises (-0.0 survives);
    # a need with no served row: NaN, and its neighbours keep their bits
    for served in ([False, True, True, True, True, True], [True, False, True, False, True, True], [True, True, False, False, False, True],
                   [True, True, True, True, True, False], [False] * 6):
        for mode in ("sum", "max"):
            got = fused_batch_ref.fuse_batch(S, offs, w, mode, served)
            assert bits(got) == bits(plain_fuse_batch(S.tolist(), offs, w.tolist(), mode, served))
    got = fused_batch_ref.fuse_batch(S, offs, w, "sum", [True, True, False, False, False, True])
    assert np.isnan(got[1]).all() and bits(got[0]) == bits(Fs[0]) and bits(got[2]) == bits(Fs[2])
    Z = np.array([[1.0], [-0.0]])
    assert bits(fused_batch_ref.fuse_batch(Z, [0, 2], np.array([1.0, 1.0]), "sum", [False, True])) == bits([[-0.0]])
