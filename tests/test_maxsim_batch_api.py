"""CPU: the surface of batched late-interaction search -- ArrowSpace.search_maxsim_batch / score_maxsim_batch /
maxsim_batch_counters (also under the reference module name), the C ABI symbols behind them, the refusals the C entries make
before they touch a handle, the argument checks the Python layer makes before it enters the library, and the numpy reference
tests/maxsim_batch_ref.py against a plain Python-float loop on hand-built score matrices.  No compute call: the GPU behaviour is
tests/test_gpu_maxsim_batch.py's."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import maxsim_batch_ref
import maxsim_ref

SYMBOLS = ("as_search_maxsim_batch", "as_score_maxsim_batch", "as_maxsim_batch_counters", "as_maxsim_batch_kernel_us")


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
        for name in ("search_maxsim_batch", "score_maxsim_batch", "maxsim_batch_counters"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
    sig = inspect.signature(asp.ArrowSpace.search_maxsim_batch)
    assert list(sig.parameters) == ["self", "needs", "gl", "tau", "groups", "n_groups", "weights", "subset", "on_zero_lambda"]
    assert sig.parameters["n_groups"].default is inspect.Parameter.empty
    assert [sig.parameters[p].default for p in ("weights", "subset", "on_zero_lambda")] == [None, None, "raise"]
    sig = inspect.signature(asp.ArrowSpace.score_maxsim_batch)
    assert list(sig.parameters) == ["self", "needs", "gl", "tau", "groups", "labels", "weights", "subset", "on_zero_lambda"]
    assert sig.parameters["labels"].default is inspect.Parameter.empty
    assert [sig.parameters[p].default for p in ("weights", "subset", "on_zero_lambda")] == [None, None, "raise"]
    assert list(inspect.signature(asp.ArrowSpace.maxsim_batch_counters).parameters) == ["self"]


def test_library_exports_the_batched_maxsim_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert '"maxsim_batch_timing"' in hdr and '"maxsim_batch_mib"' in hdr


def test_the_tuning_keys_are_known(asp):
    try:
        assert asp._L.as_set_tuning(b"maxsim_batch_timing", 1) == 0
        assert asp._L.as_set_tuning(b"maxsim_batch_mib", -8) == 0
    finally:
        assert asp._L.as_set_tuning(b"maxsim_batch_timing", 0) == 0
        assert asp._L.as_set_tuning(b"maxsim_batch_mib", 0) == 0
    assert asp._L.as_set_tuning(b"maxsim_batch_timings", 1) == 1   # an unknown key
    assert asp._L.as_set_tuning(b"maxsim_batch_mibs", 1) == 1


def test_null_and_bad_offset_arguments_are_rejected_without_a_gpu(asp):
    """Handles that point nowhere a library could read: every refusal below comes before a handle is touched."""
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    fake = ctypes.c_void_p(8)   # never dereferenced
    q = (ctypes.c_double * 12)()
    lab = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    sc = (ctypes.c_double * 4)(5.0, 5.0, 5.0, 5.0)
    ln = (ctypes.c_int64 * 2)(9, 9)
    lq = (ctypes.c_double * 3)(3.0, 3.0, 3.0)
    st = (ctypes.c_int32 * 2)(9, 9)
    listed = (ctypes.c_int64 * 2)(0, 1)
    good = (ctypes.c_int64 * 3)(0, 1, 3)

    def untouched():
        return (list(lab) == [7] * 4 and list(sc) == [5.0] * 4 and list(ln) == [9, 9] and list(lq) == [3.0] * 3 and list(st) == [9, 9])

    def search(sp, gr, qq, offs, grp, b, nv, ng=2, out_label=lab, out_score=sc, out_len=ln):
        return L.as_search_maxsim_batch(sp, gr, qq, offs, b, nv, 4, 0.5, None, 0, grp, ng, None, out_label, out_score, out_len, lq, st)

    def score(sp, gr, qq, offs, grp, b, nv, labels=listed, nl=2, out=sc):
        return L.as_score_maxsim_batch(sp, gr, qq, offs, b, nv, 4, 0.5, None, 1, grp, None, labels, nl, out, lq, st)

    for args in ((None, None, q, good, fake), (None, fake, q, good, fake), (fake, None, q, good, fake), (fake, fake, None, good, fake),
                 (fake, fake, q, None, fake), (fake, fake, q, good, None)):
        assert search(*args, 2, 3) == EINVAL
        assert "as_search_maxsim_batch: null argument" in asp._lib.last_error() and untouched()
        assert score(*args, 2, 3) == EINVAL
        assert "as_score_maxsim_batch: null argument" in asp._lib.last_error() and untouched()
    for kw in ({"out_label": None}, {"out_score": None}, {"out_len": None}):
        assert search(fake, fake, q, good, fake, 2, 3, **kw) == EINVAL and "null argument" in asp._lib.last_error() and untouched()
    for kw in ({"labels": None}, {"out": None}, {"nl": -1}):
        assert score(fake, fake, q, good, fake, 2, 3, **kw) == EINVAL and "null argument" in asp._lib.last_error() and untouched()
    # offsets: start at 0, increase strictly, end at nv; b >= 1
    bad = (((1, 2, 3), 2, 3, "start at 0"), ((0, 1, 2), 2, 3, "end at nv"), ((0, 1, 4), 2, 3, "end at nv"), ((0, 0, 3), 2, 3, "strictly"),
           ((0, 3, 3), 2, 3, "strictly"), ((0, 4, 3), 2, 3, "strictly"), ((0, 1, 3), 0, 0, "b must be"), ((0, 1, 3), -1, 3, "b must be"))
    for offs, b, nv, what in bad:
        o = (ctypes.c_int64 * 3)(*offs)
        assert search(fake, fake, q, o, fake, b, nv) == EINVAL and what in asp._lib.last_error(), (offs, asp._lib.last_error())
        assert "as_search_maxsim_batch" in asp._lib.last_error() and untouched()
        assert score(fake, fake, q, o, fake, b, nv) == EINVAL and what in asp._lib.last_error(), (offs, asp._lib.last_error())
        assert "as_score_maxsim_batch" in asp._lib.last_error() and untouched()
    # the range of n_groups is looked at before a handle is: only the lengths are reset
    for ng in (0, -1, 1025):
        ln[0] = ln[1] = 9
        assert search(fake, fake, q, good, fake, 2, 3, ng=ng) == EINVAL
        assert "as_search_maxsim_batch: n_groups must be in [1, 1024]" in asp._lib.last_error()
        assert list(ln) == [0, 0] and list(lab) == [7] * 4 and list(sc) == [5.0] * 4 and list(lq) == [3.0] * 3 and list(st) == [9, 9]
    out = (ctypes.c_int64 * 8)(1, 2, 3, 4, 5, 6, 7, 8)
    assert L.as_maxsim_batch_counters(None, out, 8) == EINVAL and list(out) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert "as_maxsim_batch_counters: null argument" in asp._lib.last_error()
    for part in (0, 1, 2, 3):
        assert L.as_maxsim_batch_kernel_us(None, part) == 0.0


def test_argument_errors_are_raised_before_the_library_is_entered(asp):
    """A space and a graph that hold no handle are enough: every refusal comes before a handle is touched."""
    space, other = object.__new__(asp.ArrowSpace), object.__new__(asp.ArrowSpace)
    gl = object.__new__(asp.GraphLaplacian)
    N = [np.zeros((3, 4)), np.zeros((1, 4))]
    mine = asp.ItemGroups._wrap(None, space, np.array([5, -2, 5, 2 ** 40, 9]))
    theirs = asp.ItemGroups._wrap(None, other, np.arange(5))
    their_sub = asp.ItemSubset._wrap(None, other)
    calls = (lambda **kw: space.search_maxsim_batch(kw.pop("needs", N), kw.pop("gl", gl), kw.pop("tau", 0.62), kw.pop("groups", mine),
                                                    kw.pop("n_groups", 3), **kw),
             lambda **kw: space.score_maxsim_batch(kw.pop("needs", N), kw.pop("gl", gl), kw.pop("tau", 0.62), kw.pop("groups", mine),
                                                   kw.pop("labels", [5, 9]), **kw))
    for call in calls:
        with pytest.raises(TypeError, match="GraphLaplacian"):
            call(gl=None)
        # ragged and 3-D needs: a need that is not 2-D (the message names it), needs that are no sequence of needs
        with pytest.raises(TypeError, match="need 1 must be a 2-D"):
            call(needs=[np.zeros((2, 4)), np.zeros(4)])
        with pytest.raises(TypeError, match="need 0 must be a 2-D"):
            call(needs=[np.zeros((2, 2, 4))])
        with pytest.raises(TypeError, match="need 1 must be a 2-D"):
            call(needs=[[[0.0, 1.0]], [[0.0, 1.0], [2.0]]])   # a ragged need
        for needs in (np.zeros((3, 4)), np.zeros(4), np.zeros((2, 2, 2, 4)), 1.0, "ab", None):
            with pytest.raises(TypeError, match="needs"):
                call(needs=needs)
        for needs in ([], np.zeros((0, 2, 4))):
            with pytest.raises(ValueError, match="at least one need"):
                call(needs=needs)
        with pytest.raises(ValueError, match="need 1 must hold at least one"):   # an empty need
            call(needs=[np.zeros((2, 4)), np.zeros((0, 4))])
        with pytest.raises(ValueError, match="at least one"):
            call(needs=np.zeros((2, 0, 4)))
        with pytest.raises(ValueError, match="need 2 has D = 5"):
            call(needs=[np.zeros((2, 4)), np.zeros((1, 4)), np.zeros((1, 5))])
        with pytest.raises(TypeError, match="mode"):   # the fold is the sum: there is no mode to choose
            call(mode="max")
        for ozl in ("ignore", "", None, True):
            with pytest.raises(ValueError, match="on_zero_lambda"):
                call(on_zero_lambda=ozl)
        # weight shapes: a wrong number of entries, a wrong weight count or rank inside a need
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
        # a None entry INSIDE a need's weights (a None entry for a whole need is the default and legal)
        for w, who in (([["a", "b", "c"], [1.0]], "need 0"), ([None, "a"], "need 1"), ([[1.0, 2.0, 3.0], [None]], "need 1"),
                       ([[1.0, None, 3.0], None], "need 0")):
            with pytest.raises(TypeError, match=f"weights.*{who}"):
                call(weights=w)
        with pytest.raises(TypeError, match="weights"):
            call(weights="ab")
        for tau in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="tau"):
                call(tau=tau)
        with pytest.raises(ValueError, match="groups.*another space"):
            call(groups=theirs)
        with pytest.raises(ValueError, match="subset.*another space"):
            call(subset=their_sub)
    for v in (1.0, "2", None, True, np.float64(2.0)):
        with pytest.raises(TypeError, match="n_groups"):
            calls[0](n_groups=v)
    for v in (0, -1, 1025, np.int64(1025)):
        with pytest.raises(ValueError, match="n_groups"):
            calls[0](n_groups=v)
    for bad, label in (([5, 7], 7), ([3], 3), (np.array([9, 2 ** 40, -2, -3]), -3), (np.array([2 ** 63], dtype=np.uint64), 2 ** 63)):
        with pytest.raises(ValueError, match=f"label {label} is not one of the groups"):
            calls[1](labels=bad)
    with pytest.raises(ValueError, match="1-D"):
        calls[1](labels=[[5, 9]])
    for bad in ([5.0, 9.0], ["5"], [None], np.array([True, False])):
        with pytest.raises(TypeError, match="labels"):
            calls[1](labels=bad)
    # what reaches the library: `search_fused_batch`'s parse of the needs and weights under the sum fold, then the grouped forms'
    A, B = np.arange(12.0).reshape(3, 4)[:, ::-1], np.arange(4.0).reshape(1, 4)
    V, offs, w, skip, tau, ng, grp, sub = space._maxsim_batch_args([A, B], gl, 1, mine, np.int64(7), [None, (np.float32(0.5),)], None, "skip")
    assert V.flags.c_contiguous and V.dtype == np.float64 and V.tolist() == np.concatenate([A, B]).tolist()
    assert offs.dtype == np.int64 and offs.tolist() == [0, 3, 4]
    assert w.dtype == np.float64 and w.tolist() == [1.0 / 3, 1.0 / 3, 1.0 / 3, 0.5]
    assert (skip, tau, ng, sub) == (1, 1.0, 7, None) and type(tau) is float and type(ng) is int and grp is mine
    assert space._maxsim_batch_args(np.zeros((5, 2, 4)), gl, 0.5, mine, 1, None, None, "raise")[2] is None


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def same_values(got, want):
    """Equal NaN positions, equal bits elsewhere."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.isnan(got).tolist() == nan.tolist() and bits(got[~nan]) == bits(want[~nan])


def plain_maxsim_batch(S, labels, offsets, w, served=None):
    """S17 in plain Python floats, one need and one group at a time -> B rows over the ascending labels."""
    out = []
    for b in range(len(offsets) - 1):
        row = []
        for g in sorted(set(labels)):
            F = None
            for v in range(offsets[b], offsets[b + 1]):
                if served is not None and not served[v]:
                    continue
                best = None
                for i, l in enumerate(labels):
                    s = float(S[v][i])
                    if l != g or math.isnan(s):
                        continue
                    if best is None or s > best:
                        best = s
                m = float("nan") if best is None else best + 0.0   # a maximum of zero is +0.0
                t = float(w[v]) * m
                F = t if F is None else F + t
            row.append(float("nan") if F is None else F)
        out.append(row)
    return out


NAN = float("nan")
LABELS = [4, -7, 4, 2 ** 41, -7, 30, 4]
#    group 4: items 0, 2, 6; group -7: items 1, 4 (a maximum of -0.0 in row 0); group 2^41: item 3; group 30: item 5, NaN throughout
S = np.array([[1.5, -0.0, NAN, 0.25, -1.0, NAN, 1.25],
              [-2.0, 3.0, -0.5, NAN, 3.0, NAN, NAN],
              [0.5, 0.75, 8.0, 1.0, NAN, NAN, -8.0],
              [-0.0, -0.0, -1.0, 2.0, -3.0, NAN, -2.0],
              [1.0, 1.0, 1.0, 1.0, 1.0, NAN, 1.0],
              [1.0, 1.0, 1.0, 1.0, 1.0, NAN, 1.0]])
W = np.array([0.5, -2.0, 0.25, 3.0, 1.0, -1.0])


def test_the_reference_on_a_hand_built_matrix():
    offs = [0, 1, 3, 4, 6]   # a need of one row first; a two-row need; a need of one row with -0.0 maxima; a +1 / -1 need
    lab, F = maxsim_batch_ref.maxsim_batch(S, LABELS, offs, W)
    assert lab.tolist() == [-7, 4, 30, 2 ** 41] and F.shape == (4, 4) and F.dtype == np.float64
    assert same_values(F, plain_maxsim_batch(S.tolist(), LABELS, offs, W.tolist()))
    # a need of one row: the first served row initialises, no 0 + t; the -0.0 maximum of group -7 became +0.0 before the product
    assert bits(F[0, :2]) == bits([0.5 * 0.0, 0.5 * 1.5]) and bits(F[0, 3:]) == bits([0.5 * 0.25])
    assert bits(F[2, :2]) == bits([3.0 * 0.0, 3.0 * 0.0]) and bits(F[2, :1]) == bits([0.0])   # -0.0 maxima: +0.0, not -0.0
    assert np.isnan(F[:, 2]).all()                      # the all-NaN group, under every need
    assert math.isnan(F[1, 3]) and F[1, 0] == -2.0 * 3.0 + 0.25 * 0.75   # no member under one vector: NaN; else the sum in row order
    assert bits(F[3, [0, 1, 3]]) == bits([0.0, 0.0, 0.0])   # +1 / -1 cancel to +0.0
    # every need is the single form over its own rows
    for b in range(4):
        l1, F1 = maxsim_ref.maxsim(S[offs[b]:offs[b + 1]], LABELS, W[offs[b]:offs[b + 1]])
        assert l1.tolist() == lab.tolist() and same_values(F[b], F1)
    tops = maxsim_batch_ref.top_batch(lab, F, 10)
    assert [t[0].tolist() for t in tops] == [[4, 2 ** 41, -7], [4, -7], [2 ** 41, -7, 4], [-7, 4, 2 ** 41]]   # NaN left out; ties by label
    assert [t[0].tolist() for t in maxsim_batch_ref.top_batch(lab, F, 1)] == [[4], [4], [2 ** 41], [-7]]
    assert maxsim_batch_ref.default_weights(offs).tolist() == [1.0, 0.5, 0.5, 1.0, 0.5, 0.5]


def test_unserved_rows_and_an_unserved_need():
    offs = [0, 3, 4, 6]
    for served in ([False, True, True, True, True, True], [True, False, True, True, True, True], [True, True, False, True, False, True],
                   [True, True, True, False, True, True], [False] * 6):
        lab, F = maxsim_batch_ref.maxsim_batch(S, LABELS, offs, W, served)
        assert same_values(F, plain_maxsim_batch(S.tolist(), LABELS, offs, W.tolist(), served)), served
    # an unserved need gives a row of NaN and an empty list, its neighbours keep their bits
    lab, whole = maxsim_batch_ref.maxsim_batch(S, LABELS, offs, W)
    lab, F = maxsim_batch_ref.maxsim_batch(S, LABELS, offs, W, [True, True, True, False, True, True])
    assert np.isnan(F[1]).all() and same_values(F[0], whole[0]) and same_values(F[2], whole[2])
    tops = maxsim_batch_ref.top_batch(lab, F, 3)
    assert tops[1][0].tolist() == [] and tops[1][1].tolist() == [] and len(tops[0][0]) == 2 and len(tops[2][0]) == 3
    with pytest.raises(ValueError):
        maxsim_batch_ref.maxsim_batch(S, LABELS, [0, 3, 3, 6], W)   # an empty need
    with pytest.raises(ValueError):
        maxsim_batch_ref.maxsim_batch(S, LABELS, [0, 3, 5], W)      # offsets do not end at the rows


def test_the_reference_agrees_with_a_plain_loop_on_random_arrays():
    rng = np.random.default_rng(17)
    for Js, m, nlab in (((1,), 1, 1), ((2, 1, 5), 40, 5), ((3, 3, 3), 60, 60), ((1, 9, 2), 300, 17)):
        offs = np.concatenate([[0], np.cumsum(Js)]).tolist()
        labels = rng.integers(-3, nlab - 3, m)
        Sr = np.round(rng.standard_normal((offs[-1], m)), 1)   # many ties and zeros
        Sr[rng.random(Sr.shape) < 0.1] = NAN
        Sr[Sr == 0.0] = -0.0
        w = rng.uniform(-1.0, 1.0, offs[-1])
        lab, F = maxsim_batch_ref.maxsim_batch(Sr, labels, offs, w)
        assert lab.tolist() == sorted(set(labels.tolist()))
        assert same_values(F, plain_maxsim_batch(Sr.tolist(), labels.tolist(), offs, w.tolist()))
