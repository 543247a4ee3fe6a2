"""CPU: the surface of grouped search -- ArrowSpace.groups / search_grouped / search_batch_grouped / grouped_counters and
ItemGroups (also under the reference module name), the C ABI symbols behind them, the argument checks the Python layer makes
before it enters the library, and the numpy reference tests/grouped_ref.py against a plain Python loop.  No compute call: the
GPU behaviour is tests/test_gpu_grouped.py's."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import grouped_ref

SYMBOLS = ("as_groups_create", "as_groups_count", "as_groups_free", "as_search_grouped", "as_search_grouped_batch",
           "as_grouped_counters", "as_grouped_kernel_us")


@pytest.fixture(scope="module")
def asp():
    import __graft_entry__ as g
    g.build()
    import pyarrowspace_amd
    return pyarrowspace_amd


def test_methods_exist_under_both_module_names(asp):
    import arrowspace
    assert arrowspace.ArrowSpace is asp.ArrowSpace
    assert arrowspace.ItemGroups is asp.ItemGroups and "ItemGroups" in asp.__all__
    for mod in (asp, arrowspace):
        for name in ("groups", "search_grouped", "search_batch_grouped", "grouped_counters"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
    for name in ("search_grouped", "search_batch_grouped"):
        sig = inspect.signature(getattr(asp.ArrowSpace, name))
        first = "item" if name == "search_grouped" else "items"
        assert list(sig.parameters) == ["self", first, "gl", "tau", "groups", "n_groups", "per_group", "subset"]
        assert sig.parameters["n_groups"].default is inspect.Parameter.empty
        assert [sig.parameters[p].default for p in ("per_group", "subset")] == [1, None]
    assert list(inspect.signature(asp.ArrowSpace.groups).parameters) == ["self", "labels"]
    assert asp.ItemGroups.__doc__.startswith("Extension:")
    for name in ("ngroups", "labels", "__len__"):
        assert hasattr(asp.ItemGroups, name), name
    with pytest.raises(ValueError, match="cannot be constructed directly; use ArrowSpace.groups"):
        asp.ItemGroups()
    assert asp.GROUPED_MAX_PER_GROUP == 16 and asp.GROUPED_MAX_GROUPS == 1024


def test_library_exports_the_grouped_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert '"grouped_timing"' in hdr


def test_null_arguments_are_rejected_without_a_gpu(asp):
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    q = (ctypes.c_double * 8)()
    lab = (ctypes.c_int64 * 2)(7, 7)
    cnt = (ctypes.c_int64 * 2)(6, 6)
    idx = (ctypes.c_int64 * 2)(5, 5)
    sc = (ctypes.c_double * 2)(4.0, 4.0)
    n = (ctypes.c_int64 * 2)(9, 9)
    lq = (ctypes.c_double * 2)(3.0, 3.0)
    st = (ctypes.c_int32 * 2)(8, 8)

    def untouched():
        return (list(lab), list(cnt), list(idx), list(sc), list(n), list(lq), list(st)) == (
            [7, 7], [6, 6], [5, 5], [4.0, 4.0], [9, 9], [3.0, 3.0], [8, 8])

    assert L.as_search_grouped(None, None, q, 8, 0.5, None, 2, 1, None, lab, cnt, idx, sc, n, lq) == EINVAL
    assert "as_search_grouped: null argument" in asp._lib.last_error() and untouched()
    assert L.as_search_grouped_batch(None, None, q, 2, 4, 0.5, None, 1, 1, None, lab, cnt, idx, sc, n, lq, st) == EINVAL
    assert "as_search_grouped_batch: null argument" in asp._lib.last_error() and untouched()
    h = ctypes.c_void_p(1234)
    assert L.as_groups_create(None, lab, 2, ctypes.byref(h)) == EINVAL and h.value == 1234
    assert "as_groups_create: null argument" in asp._lib.last_error()
    assert L.as_groups_count(None) == 0
    L.as_groups_free(None)
    out = (ctypes.c_int64 * 7)(1, 2, 3, 4, 5, 6, 7)
    assert L.as_grouped_counters(None, out, 7) == EINVAL and list(out) == [1, 2, 3, 4, 5, 6, 7]
    assert "as_grouped_counters: null argument" in asp._lib.last_error()
    assert L.as_grouped_kernel_us(None) == 0.0


def test_timing_is_a_tuning_key(asp):
    try:
        assert asp._L.as_set_tuning(b"grouped_timing", 1) == 0
    finally:
        assert asp._L.as_set_tuning(b"grouped_timing", 0) == 0
    assert asp._L.as_set_tuning(b"grouped_timings", 1) == 1   # an unknown key


def test_argument_errors_are_raised_before_the_library_is_entered(asp):
    """A space and a graph that hold no handle are enough: every refusal comes before a handle is touched."""
    space, other = object.__new__(asp.ArrowSpace), object.__new__(asp.ArrowSpace)
    gl = object.__new__(asp.GraphLaplacian)
    q, Q = np.zeros(4), np.zeros((3, 4))
    mine = asp.ItemGroups._wrap(None, space, np.arange(5))
    theirs = asp.ItemGroups._wrap(None, other, np.arange(5))
    their_sub = asp.ItemSubset._wrap(None, other)
    calls = (lambda **kw: space.search_grouped(kw.pop("item", q), kw.pop("gl", gl), kw.pop("tau", 0.62), kw.pop("groups", mine),
                                               kw.pop("n_groups", 3), **kw),
             lambda **kw: space.search_batch_grouped(kw.pop("item", Q), kw.pop("gl", gl), kw.pop("tau", 0.62), kw.pop("groups", mine),
                                                     kw.pop("n_groups", 3), **kw))
    for call in calls:
        with pytest.raises(TypeError, match="GraphLaplacian"):
            call(gl=None)
        for name, top in (("n_groups", 1024), ("per_group", 16)):
            for v in (1.0, "2", None, True, np.float64(2.0)):
                with pytest.raises(TypeError, match=name):
                    call(**{name: v})
            for v in (0, -1, top + 1, np.int64(top + 1)):
                with pytest.raises(ValueError, match=name):
                    call(**{name: v})
        for tau in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="tau"):
                call(tau=tau)
        with pytest.raises(ValueError, match="groups.*another space"):
            call(groups=theirs)
        with pytest.raises(ValueError, match="subset.*another space"):
            call(subset=their_sub)
    for bad in (np.zeros(4, dtype=np.float32), [0.0] * 4, np.zeros((2, 4))):
        with pytest.raises(TypeError, match="item"):
            calls[0](item=bad)
    with pytest.raises(ValueError, match="contiguous"):
        calls[0](item=np.zeros(8)[::2])
    for bad in (np.zeros(4), np.zeros((2, 2, 2))):
        with pytest.raises(TypeError, match="2-D"):
            calls[1](item=bad)
    assert space.search_batch_grouped(np.zeros((0, 4)), gl, 0.62, mine, 3) == []   # B = 0: nothing is launched
    # the labels of groups(): dtype, rank and length
    for bad in (np.zeros(5), np.zeros(5, dtype=bool), [0.5] * 5, ["a"] * 5, [None] * 5):
        with pytest.raises(TypeError, match="labels"):
            asp._group_labels(bad, 5)
    for bad in (np.arange(4), np.arange(6), np.zeros((5, 1), dtype=np.int64), 3, np.array([2 ** 63] * 5, dtype=np.uint64)):
        with pytest.raises(ValueError, match="labels"):
            asp._group_labels(bad, 5)
    lab = asp._group_labels([3, -1, 2 ** 40, 3, 0], 5)
    assert lab.dtype == np.int64 and lab.flags.c_contiguous and lab.tolist() == [3, -1, 2 ** 40, 3, 0]
    assert asp._group_labels(np.array([1, 2, 3, 4, 5], dtype=np.uint8), 5).tolist() == [1, 2, 3, 4, 5]
    got = mine.labels()
    got[0] = 99
    assert mine.labels().tolist() == [0, 1, 2, 3, 4]   # a copy


def plain_grouped(ids, labels, scores, n_groups, per_group):
    """S14 in plain Python: the items in order, then group after group."""
    items = [(i, l, s) for i, l, s in zip(ids, labels, scores) if not math.isnan(s)]
    rest = sorted(items, key=lambda e: (-(e[2] + 0.0), e[0]))
    out = []
    while rest and len(out) < n_groups:
        head = rest[0]
        members = [(i, s) for i, l, s in rest if l == head[1]]
        out.append((head[1], members[:per_group]))
        rest = [e for e in rest if e[1] != head[1]]
    return out


def same(a, b):
    """Equal labels, indices and score bits."""
    flat = lambda r: [(l, [(i, np.float64(s).view(np.uint64)) for i, s in mem]) for l, mem in r]
    return flat(a) == flat(b)


NAN = float("nan")


def test_the_reference_agrees_with_a_plain_loop_on_hand_written_arrays():
    ids = [2, 3, 5, 7, 8, 11, 12, 13, 17, 19]
    labels = [-4, 9, -4, 9, 2 ** 41, 6, 6, -4, 2 ** 41, 30]
    #        equal scores inside group -4 (2, 5) and between the heads of -4 and 9 (2, 3); -0.0 / +0.0 in group 6; a NaN
    scores = [1.5, 1.5, 1.5, 0.25, NAN, 0.0, -0.0, -2.0, 0.75, NAN]
    for ng in (1, 2, 3, 4, 5, 1024):
        for pg in (1, 2, 3, 16):
            got = grouped_ref.grouped(ids, labels, scores, ng, pg)
            assert same(got, plain_grouped(ids, labels, scores, ng, pg)), (ng, pg)
    got = grouped_ref.grouped(ids, labels, scores, 1024, 16)
    assert [l for l, _ in got] == [-4, 9, 2 ** 41, 6]   # label 30 has only a NaN: it does not exist; n_groups beyond the groups
    assert [i for i, _ in got[0][1]] == [2, 5, 13]      # per_group beyond the group: the whole group
    assert [i for i, _ in got[1][1]] == [3, 7]
    assert got[2][1] == [(17, 0.75)]                    # item 8 (NaN) is no member
    assert [i for i, _ in got[3][1]] == [11, 12]        # -0.0 ties with +0.0: index order ...
    assert math.copysign(1.0, got[3][1][1][1]) == -1.0  # ... and the score keeps its sign bit
    assert grouped_ref.grouped(ids, labels, scores, 2, 1) == [(-4, [(2, 1.5)]), (9, [(3, 1.5)])]
    assert grouped_ref.grouped([], [], [], 3, 2) == [] and grouped_ref.grouped([1], [0], [NAN], 3, 2) == []


def test_the_reference_agrees_with_a_plain_loop_on_random_arrays():
    rng = np.random.default_rng(14)
    for m, nlab in ((1, 1), (40, 5), (200, 200), (300, 17)):
        ids = np.sort(rng.choice(1000, m, replace=False))
        labels = rng.integers(-3, nlab - 3, m)
        scores = np.round(rng.standard_normal(m), 1)   # many ties
        scores[rng.random(m) < 0.05] = NAN
        for ng, pg in ((1, 1), (3, 2), (1024, 16)):
            assert same(grouped_ref.grouped(ids, labels, scores, ng, pg), plain_grouped(ids.tolist(), labels.tolist(), scores.tolist(), ng, pg))
