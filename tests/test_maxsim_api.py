"""CPU: the surface of late-interaction search -- ArrowSpace.search_maxsim / score_maxsim / maxsim_counters (also under the
reference module name), the C ABI symbols behind them, the argument checks the Python layer makes before it enters the library,
and the numpy reference tests/maxsim_ref.py against a plain Python loop.  No compute call: the GPU behaviour is
tests/test_gpu_maxsim.py's."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import maxsim_ref

SYMBOLS = ("as_search_maxsim", "as_score_maxsim", "as_maxsim_counters", "as_maxsim_kernel_us")


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
        for name in ("search_maxsim", "score_maxsim", "maxsim_counters"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
    sig = inspect.signature(asp.ArrowSpace.search_maxsim)
    assert list(sig.parameters) == ["self", "items", "gl", "tau", "groups", "n_groups", "weights", "subset", "on_zero_lambda"]
    assert sig.parameters["n_groups"].default is inspect.Parameter.empty
    assert [sig.parameters[p].default for p in ("weights", "subset", "on_zero_lambda")] == [None, None, "raise"]
    sig = inspect.signature(asp.ArrowSpace.score_maxsim)
    assert list(sig.parameters) == ["self", "items", "gl", "tau", "groups", "labels", "weights", "subset", "on_zero_lambda"]
    assert sig.parameters["labels"].default is inspect.Parameter.empty
    assert [sig.parameters[p].default for p in ("weights", "subset", "on_zero_lambda")] == [None, None, "raise"]


def test_library_exports_the_maxsim_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert '"maxsim_timing"' in hdr


def test_null_and_out_of_range_arguments_are_rejected_without_a_gpu(asp):
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    q = (ctypes.c_double * 8)()
    lab = (ctypes.c_int64 * 2)(7, 7)
    sc = (ctypes.c_double * 2)(5.0, 5.0)
    ln = ctypes.c_int64(9)
    lq = (ctypes.c_double * 2)(3.0, 3.0)
    st = (ctypes.c_int32 * 2)(9, 9)

    def untouched():
        return (list(lab), list(sc), ln.value, list(lq), list(st)) == ([7, 7], [5.0, 5.0], 9, [3.0, 3.0], [9, 9])

    assert L.as_search_maxsim(None, None, q, 2, 4, 0.5, None, 0, None, 2, None, lab, sc, ctypes.byref(ln), lq, st) == EINVAL
    assert "as_search_maxsim: null argument" in asp._lib.last_error() and untouched()
    assert L.as_score_maxsim(None, None, q, 2, 4, 0.5, None, 1, None, None, lab, 2, sc, lq, st) == EINVAL
    assert "as_score_maxsim: null argument" in asp._lib.last_error() and untouched()
    # handles that are never dereferenced: the range of n_groups and the count of labels are looked at first
    fake = ctypes.c_void_p(8)
    for ng in (0, -1, 1025):
        ln.value = 9
        assert L.as_search_maxsim(fake, fake, q, 2, 4, 0.5, None, 0, fake, ng, None, lab, sc, ctypes.byref(ln), lq, st) == EINVAL
        assert "n_groups must be in [1, 1024]" in asp._lib.last_error() and ln.value == 0
    ln.value = 9
    assert L.as_score_maxsim(fake, fake, q, 2, 4, 0.5, None, 0, fake, None, lab, -1, sc, lq, st) == EINVAL
    assert L.as_score_maxsim(fake, fake, q, 2, 4, 0.5, None, 0, fake, None, None, 2, sc, lq, st) == EINVAL
    assert "as_score_maxsim: null argument" in asp._lib.last_error() and untouched()
    out = (ctypes.c_int64 * 5)(1, 2, 3, 4, 5)
    assert L.as_maxsim_counters(None, out, 5) == EINVAL and list(out) == [1, 2, 3, 4, 5]
    assert "as_maxsim_counters: null argument" in asp._lib.last_error()
    for part in (0, 1, 2, 3):
        assert L.as_maxsim_kernel_us(None, part) == 0.0


def test_timing_is_a_tuning_key(asp):
    try:
        assert asp._L.as_set_tuning(b"maxsim_timing", 1) == 0
    finally:
        assert asp._L.as_set_tuning(b"maxsim_timing", 0) == 0
    assert asp._L.as_set_tuning(b"maxsim_timings", 1) == 1   # an unknown key


def test_argument_errors_are_raised_before_the_library_is_entered(asp):
    """A space and a graph that hold no handle are enough: every refusal comes before a handle is touched."""
    space, other = object.__new__(asp.ArrowSpace), object.__new__(asp.ArrowSpace)
    gl = object.__new__(asp.GraphLaplacian)
    Q = np.zeros((3, 4))
    mine = asp.ItemGroups._wrap(None, space, np.array([5, -2, 5, 2 ** 40, 9]))
    theirs = asp.ItemGroups._wrap(None, other, np.arange(5))
    their_sub = asp.ItemSubset._wrap(None, other)
    calls = (lambda **kw: space.search_maxsim(kw.pop("items", Q), kw.pop("gl", gl), kw.pop("tau", 0.62), kw.pop("groups", mine),
                                              kw.pop("n_groups", 3), **kw),
             lambda **kw: space.score_maxsim(kw.pop("items", Q), kw.pop("gl", gl), kw.pop("tau", 0.62), kw.pop("groups", mine),
                                             kw.pop("labels", [5, 9]), **kw))
    for call in calls:
        with pytest.raises(TypeError, match="GraphLaplacian"):
            call(gl=None)
        with pytest.raises(TypeError, match="2-D"):
            call(items=np.zeros(4))
        with pytest.raises(ValueError, match="at least one"):
            call(items=np.zeros((0, 4)))
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


def plain_maxsim(S, labels, w, served=None):
    """S16 in plain Python floats, one group at a time -> {label: F}."""
    out = {}
    for g in sorted(set(labels)):
        F = None
        for j in range(len(S)):
            if served is not None and not served[j]:
                continue
            best = None
            for i, l in enumerate(labels):
                s = float(S[j][i])
                if l != g or math.isnan(s):
                    continue
                if best is None or s > best:
                    best = s
            m = float("nan") if best is None else best + 0.0   # a maximum of zero is +0.0
            t = float(w[j]) * m
            F = t if F is None else F + t
        out[g] = F
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def same_values(got, want):
    """Equal NaN positions, equal bits elsewhere."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.isnan(got).tolist() == nan.tolist() and bits(got[~nan]) == bits(want[~nan])


NAN = float("nan")


def test_the_reference_agrees_with_a_plain_loop_on_a_hand_built_matrix():
    labels = [4, -7, 4, 2 ** 41, -7, 30, 4]
    #    group 4: items 0, 2, 6; group -7: items 1, 4 (a maximum of -0.0 in row 0); group 2^41: item 3; group 30: item 5, NaN throughout
    S = np.array([[1.5, -0.0, NAN, 0.25, -1.0, NAN, 1.25],
                  [-2.0, 3.0, -0.5, NAN, 3.0, NAN, NAN],
                  [0.5, 0.75, 8.0, 1.0, NAN, NAN, -8.0]])
    w = np.array([0.5, -2.0, 0.25])
    lab, M = maxsim_ref.group_max(S, labels)
    assert lab.tolist() == [-7, 4, 30, 2 ** 41]
    assert same_values(M, [[0.0, 1.5, NAN, 0.25], [3.0, -0.5, NAN, NAN], [0.75, 8.0, NAN, 1.0]])
    assert bits(M[0, :1]) == bits([0.0])                       # the -0.0 maximum came out as +0.0
    for served in (None, [True, False, True], [False, True, True], [False, False, True]):   # an unserved row: first, middle, both
        lab, F = maxsim_ref.maxsim(S, labels, w, served)
        want = plain_maxsim(S.tolist(), labels, w.tolist(), served)
        assert same_values(F, [want[l] for l in lab.tolist()]), served
    lab, F = maxsim_ref.maxsim(S, labels, w)
    assert math.isnan(F[2]) and math.isnan(F[3])               # the all-NaN group; a group without a member under one vector
    assert F[0] == 0.5 * 0.0 + -2.0 * 3.0 + 0.25 * 0.75 and F[1] == 0.5 * 1.5 + -2.0 * -0.5 + 0.25 * 8.0
    tl, tf = maxsim_ref.top(lab, F, 10)
    assert tl.tolist() == [4, -7] and tf.tolist() == [F[1], F[0]]   # NaN left out, n beyond the groups
    assert maxsim_ref.top(lab, F, 1)[0].tolist() == [4]
    with pytest.raises(ValueError, match="served"):
        maxsim_ref.maxsim(S, labels, w, [False] * 3)
    with pytest.raises(ValueError, match="belong together"):
        maxsim_ref.group_max(S, labels[:-1])


def test_top_orders_ties_by_label_and_zeros_of_either_sign_tie():
    tl, tf = maxsim_ref.top([9, -4, 7, 1, 3], [0.5, 2.0, 0.5, NAN, 2.0], 4)
    assert tl.tolist() == [-4, 3, 7, 9] and tf.tolist() == [2.0, 2.0, 0.5, 0.5]
    assert maxsim_ref.top([2, 1], [0.0, -0.0], 2)[0].tolist() == [1, 2]


def test_the_reference_agrees_with_a_plain_loop_on_random_arrays():
    rng = np.random.default_rng(16)
    for J, m, nlab in ((1, 1, 1), (3, 40, 5), (9, 60, 60), (4, 300, 17)):
        labels = rng.integers(-3, nlab - 3, m)
        S = np.round(rng.standard_normal((J, m)), 1)   # many ties and zeros
        S[rng.random((J, m)) < 0.1] = NAN
        S[S == 0.0] = -0.0
        w = rng.uniform(-1.0, 1.0, J)
        lab, F = maxsim_ref.maxsim(S, labels, w)
        want = plain_maxsim(S.tolist(), labels.tolist(), w.tolist())
        assert same_values(F, [want[l] for l in lab.tolist()])
