"""CPU: the surface of late-interaction re-ranking of per-need candidate documents --
ArrowSpace.search_maxsim_lists / score_maxsim_lists / maxsim_lists_counters (also under the reference module name), the C ABI
symbols behind them, the refusals the C entries make before they touch a handle, the argument checks the Python layer makes before
it enters the library, the label-to-member expansion on hand-built labels, and the numpy reference tests/maxsim_lists_ref.py on
hand-built score arrays.  No compute call: the GPU behaviour is tests/test_gpu_maxsim_lists.py's."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import maxsim_lists_ref

SYMBOLS = ("as_search_maxsim_lists", "as_score_maxsim_lists", "as_maxsim_lists_counters", "as_maxsim_lists_kernel_us",
           "as_maxsim_lists_geometry")


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
        for name in ("search_maxsim_lists", "score_maxsim_lists", "maxsim_lists_counters", "maxsim_lists_geometry"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
    sig = inspect.signature(asp.ArrowSpace.search_maxsim_lists)
    assert list(sig.parameters) == ["self", "needs", "gl", "tau", "groups", "n_groups", "lists", "weights", "on_zero_lambda"]
    assert sig.parameters["lists"].default is inspect.Parameter.empty
    assert [sig.parameters[p].default for p in ("weights", "on_zero_lambda")] == [None, "raise"]
    sig = inspect.signature(asp.ArrowSpace.score_maxsim_lists)
    assert list(sig.parameters) == ["self", "needs", "gl", "tau", "groups", "lists", "weights", "on_zero_lambda"]
    assert [sig.parameters[p].default for p in ("weights", "on_zero_lambda")] == [None, "raise"]
    assert list(inspect.signature(asp.ArrowSpace.maxsim_lists_counters).parameters) == ["self"]


def test_library_exports_the_symbols_and_knows_the_tuning_key(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert '"maxsim_lists_timing"' in hdr
    try:
        assert asp._L.as_set_tuning(b"maxsim_lists_timing", 1) == 0
    finally:
        assert asp._L.as_set_tuning(b"maxsim_lists_timing", 0) == 0
    assert asp._L.as_set_tuning(b"maxsim_lists_timings", 1) == 1   # an unknown key


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
    good = (ctypes.c_int64 * 3)(0, 1, 3)
    nd = (ctypes.c_int64 * 3)(0, 1, 2)
    dl = (ctypes.c_int64 * 2)(0, 1)
    df = (ctypes.c_int64 * 3)(0, 1, 2)
    ids = (ctypes.c_int64 * 2)(0, 1)

    def untouched(lengths=(9, 9)):
        return (list(lab) == [7] * 4 and list(sc) == [5.0] * 4 and list(ln) == list(lengths) and list(lq) == [3.0] * 3 and list(st) == [9, 9])

    def search(sp, gr, qq, offs, grp, need_docs, b, nv, ng=2, out_label=lab, out_score=sc, out_len=ln):
        return L.as_search_maxsim_lists(sp, gr, qq, offs, b, nv, 4, 0.5, None, 0, grp, ng, need_docs, dl, df, ids, out_label, out_score, out_len,
                                        lq, st)

    def score(sp, gr, qq, offs, grp, need_docs, b, nv):
        return L.as_score_maxsim_lists(sp, gr, qq, offs, b, nv, 4, 0.5, None, 1, grp, need_docs, dl, df, ids, sc, lq, st)

    for args in ((None, fake, q, good, fake, nd), (fake, None, q, good, fake, nd), (fake, fake, None, good, fake, nd),
                 (fake, fake, q, None, fake, nd), (fake, fake, q, good, None, nd), (fake, fake, q, good, fake, None)):
        assert search(*args, 2, 3) == EINVAL
        assert "as_search_maxsim_lists: null argument" in asp._lib.last_error() and untouched()
        assert score(*args, 2, 3) == EINVAL
        assert "as_score_maxsim_lists: null argument" in asp._lib.last_error() and untouched()
    for kw in ({"out_label": None}, {"out_score": None}, {"out_len": None}):
        assert search(fake, fake, q, good, fake, nd, 2, 3, **kw) == EINVAL and "null argument" in asp._lib.last_error() and untouched()
    bad = (((1, 2, 3), 2, 3, "start at 0"), ((0, 1, 2), 2, 3, "end at nv"), ((0, 0, 3), 2, 3, "strictly"), ((0, 4, 3), 2, 3, "strictly"),
           ((0, 1, 3), 0, 0, "b must be"), ((0, 1, 3), -1, 3, "b must be"))
    for offs, b, nv, what in bad:
        o = (ctypes.c_int64 * 3)(*offs)
        assert search(fake, fake, q, o, fake, nd, b, nv) == EINVAL and what in asp._lib.last_error(), (offs, asp._lib.last_error())
        assert "as_search_maxsim_lists" in asp._lib.last_error() and untouched()
        assert score(fake, fake, q, o, fake, nd, b, nv) == EINVAL and what in asp._lib.last_error(), (offs, asp._lib.last_error())
        assert "as_score_maxsim_lists" in asp._lib.last_error() and untouched()
    # the range of n_groups is looked at before a handle is: only the lengths are reset
    for ng in (0, -1, 1025):
        ln[0] = ln[1] = 9
        assert search(fake, fake, q, good, fake, nd, 2, 3, ng=ng) == EINVAL and "n_groups must be in [1, 1024]" in asp._lib.last_error()
        assert untouched((0, 0))
    assert L.as_maxsim_lists_counters(None, (ctypes.c_int64 * 9)(), 9) == EINVAL
    assert L.as_maxsim_lists_kernel_us(None, 0) == 0.0
    assert L.as_maxsim_lists_geometry(None, None, None) == EINVAL


class _Gl:
    pass


def _fake_space(asp):
    sp = object.__new__(asp.ArrowSpace)
    sp._h = None
    return sp


def _fake_gl(asp):
    return object.__new__(asp.GraphLaplacian)


def test_python_checks_raise_before_a_handle_is_touched(asp):
    """A space and a graph without handles: any call that reached the library would fail on them in another way."""
    sp, gl = _fake_space(asp), _fake_gl(asp)
    needs = [np.zeros((2, 4)), np.zeros((1, 4))]
    lists = [[0, 1], [2]]
    grp = object.__new__(asp.ItemGroups)
    grp._h, grp._space, grp._labels = None, sp, np.array([0, 0, 1, 2, 2, 5], dtype=np.int64)
    cases = (
        (TypeError, "GraphLaplacian", dict(gl=None)),
        (ValueError, "on_zero_lambda", dict(on_zero_lambda="ignore")),
        (ValueError, "at least one need", dict(needs=[])),
        (TypeError, "need 1", dict(needs=[np.zeros((2, 4)), np.zeros(4)])),
        (ValueError, "same D", dict(needs=[np.zeros((2, 4)), np.zeros((1, 5))])),
        (ValueError, "weights", dict(weights=[[1.0, 2.0]])),
        (ValueError, "finite", dict(weights=[[1.0, np.nan], None])),
        (TypeError, "n_groups", dict(n_groups=2.0)),
        (ValueError, r"n_groups': must be in \[1, 1024\]", dict(n_groups=0)),
        (ValueError, r"n_groups': must be in \[1, 1024\]", dict(n_groups=1025)),
        (ValueError, "tau", dict(tau=float("nan"))),
        (ValueError, "3 label lists for 2 needs", dict(lists=[[0], [1], [2]])),
        (ValueError, "1 label lists for 2 needs", dict(lists=np.array([[0, 1]]))),
        (TypeError, "integer group labels", dict(lists=[[0.0, 1.0], [2]])),
        (TypeError, "integer group labels", dict(lists=[[True, False], [2]])),
        (TypeError, "integer group labels", dict(lists=np.zeros((2, 2)))),
        (TypeError, "sequence", dict(lists=7)),
        (ValueError, "1-D", dict(lists=[[[0, 1]], [2]])),
        (ValueError, "label 3 is not one of the groups", dict(lists=[[0, 3], [2]])),
        (ValueError, "label -9 is not one of the groups", dict(lists=np.array([[0, 1], [2, -9]]))),
    )
    for exc, match, kw in cases:
        a = dict(needs=needs, gl=gl, tau=0.5, groups=grp, n_groups=3, lists=lists, weights=None, on_zero_lambda="raise")
        a.update(kw)
        with pytest.raises(exc, match=match):
            sp.search_maxsim_lists(a["needs"], a["gl"], a["tau"], a["groups"], a["n_groups"], a["lists"], a["weights"], a["on_zero_lambda"])
        if "n_groups" in kw:
            continue
        with pytest.raises(exc, match=match):
            sp.score_maxsim_lists(a["needs"], a["gl"], a["tau"], a["groups"], a["lists"], a["weights"], a["on_zero_lambda"])
    other = object.__new__(asp.ItemGroups)
    other._h, other._space, other._labels = None, _fake_space(asp), grp._labels
    with pytest.raises(ValueError, match="another space"):
        sp.search_maxsim_lists(needs, gl, 0.5, other, 3, lists)
    with pytest.raises(ValueError, match="another space"):
        sp.score_maxsim_lists(needs, gl, 0.5, other, lists)
    grp._h = other._h = None   # (nothing to free)


def test_the_member_table_and_the_expansion_of_documents(asp):
    labels = np.array([7, -3, 7, 2 ** 40, -3, 7, 5, 2 ** 40], dtype=np.int64)
    uniq, order, starts = asp._group_members(labels)
    assert uniq.tolist() == [-3, 5, 7, 2 ** 40] and starts.tolist() == [0, 2, 3, 6, 8]
    assert order.tolist() == [1, 4, 6, 0, 2, 5, 3, 7]   # by (label, item id)
    assert uniq.dtype == order.dtype == starts.dtype == np.int64
    # order, duplicates, an empty list, a document shared by needs, a need that covers every document
    parts = asp._label_lists([[7, -3, 7], [], [2 ** 40], [5, 7, -3, 2 ** 40, 5], [7]], 5)
    assert [p.tolist() for p in parts] == [[7, -3, 7], [], [2 ** 40], [5, 7, -3, 2 ** 40, 5], [7]]
    need_docs, doc_label, doc_first, ids, inverse = asp._expand_documents(parts, (uniq, order, starts))
    assert need_docs.tolist() == [0, 2, 2, 3, 7, 8]
    assert doc_label.tolist() == [-3, 7, 2 ** 40, -3, 5, 7, 2 ** 40, 7]
    assert doc_first.tolist() == [0, 2, 5, 7, 9, 10, 13, 15, 18]
    assert ids.tolist() == [1, 4, 0, 2, 5, 3, 7, 1, 4, 6, 0, 2, 5, 3, 7, 0, 2, 5]
    assert [iv.tolist() for iv in inverse] == [[1, 0, 1], [], [0], [1, 2, 0, 3, 1], [0]]
    assert all(a.dtype == np.int64 and a.flags["C_CONTIGUOUS"] for a in (need_docs, doc_label, doc_first, ids))
    # the reference's own expansion agrees
    for b, wanted in enumerate([[7, -3, 7], [], [2 ** 40], [5, 7, -3, 2 ** 40, 5], [7]]):
        e0, e1 = doc_first[need_docs[b]], doc_first[need_docs[b + 1]]
        assert maxsim_lists_ref.members(labels, wanted).tolist() == ids[e0:e1].tolist()
    # a permutation of a list and duplicates in it change the inverse alone
    a = asp._expand_documents(asp._label_lists([[5, 7, -3]], 1), (uniq, order, starts))
    b = asp._expand_documents(asp._label_lists([[-3, 5, 5, 7, -3]], 1), (uniq, order, starts))
    assert all(x.tolist() == y.tolist() for x, y in zip(a[:4], b[:4]))
    assert a[4][0].tolist() == [1, 2, 0] and b[4][0].tolist() == [0, 1, 1, 2, 0]
    # a (B, C) array, no list at all, an unknown label, no group at all
    parts = asp._label_lists(np.array([[5, 7], [7, 7]], dtype=np.int32), 2)
    assert [p.tolist() for p in parts] == [[5, 7], [7, 7]] and all(p.dtype == np.int64 for p in parts)
    none = asp._expand_documents(asp._label_lists([[], []], 2), (uniq, order, starts))
    assert none[0].tolist() == [0, 0, 0] and none[1].size == 0 and none[2].tolist() == [0] and none[3].size == 0
    with pytest.raises(ValueError, match="label 6 is not one of the groups"):
        asp._expand_documents(asp._label_lists([[5, 6]], 1), (uniq, order, starts))
    with pytest.raises(ValueError, match="label 1 is not one of the groups"):
        asp._expand_documents(asp._label_lists([[1]], 1), asp._group_members(np.empty(0, dtype=np.int64)))
    with pytest.raises(ValueError, match="not one of the groups"):
        asp._label_lists([np.array([2 ** 63 + 5], dtype=np.uint64)], 1)


def _plain_fold(rows, w):
    """The S13 sum with Python floats: the first served term, then F + t."""
    f = None
    for s, wj in zip(rows, w):
        t = wj * s
        f = t if f is None else f + t
    return f


def test_the_reference_on_hand_built_scores():
    nan = float("nan")
    # need 0: three vectors over five entries of labels 4, 4, 9, 9, 9: a NaN beside numbers, a maximum of -0.0 and +0.0, all NaN
    S0 = np.array([[0.25, nan, -0.0, -1.0, -0.5],
                   [nan, 0.5, nan, nan, nan],
                   [0.1, 0.7, 0.0, -0.0, -3.0]])
    l0 = np.array([4, 4, 9, 9, 9])
    # need 1: one vector over entries that arrive out of label order; need 2: no entry; need 3: nothing served
    S1 = np.array([[1.0, 3.0, 2.0, -4.0]])
    l1 = np.array([8, 2, 8, 2])
    S2 = np.empty((2, 0))
    l2 = np.empty(0, dtype=np.int64)
    S3 = np.array([[0.5, 0.25], [0.75, 1.0]])
    l3 = np.array([1, 6])
    w = [np.array([0.1, 0.7, 0.3]), np.array([2.0]), np.array([0.5, 0.5]), np.array([0.5, 0.5])]
    served = [[True, True, True], [True], [True, True], [False, False]]
    out = maxsim_lists_ref.maxsim_lists([S0, S1, S2, S3], [l0, l1, l2, l3], w, served)
    lab, F = out[0]
    assert lab.tolist() == [4, 9]
    # group 4: maxima 0.25, 0.5, 0.7; group 9: maxima +0.0 (of -0.0, -1.0, -0.5), NaN (all NaN), +0.0
    assert F[0] == _plain_fold([0.25, 0.5, 0.7], w[0]) and math.isnan(F[1])
    lab, F = maxsim_lists_ref.maxsim_lists([S0], [l0], [w[0]], [[True, False, True]])[0]
    assert F[0] == _plain_fold([0.25, 0.7], [0.1, 0.3]) and F[1] == 0.0 and not math.copysign(1.0, F[1]) < 0   # +0.0
    # the fold order: (a + b) + c with every product rounded, not a dot product
    big = np.array([[1e16], [1.0], [-1e16]])
    lab, F = maxsim_lists_ref.maxsim_lists([big], [np.array([3])], [np.array([1.0, 1.0, 1.0])])[0]
    assert F[0] == (1e16 + 1.0) - 1e16 == 0.0
    lab, F = out[1]
    assert lab.tolist() == [2, 8] and F.tolist() == [6.0, 4.0]
    lab, F = out[2]
    assert lab.size == 0 and F.size == 0
    lab, F = out[3]
    assert lab.tolist() == [1, 6] and np.isnan(F).all()
    tops = maxsim_lists_ref.top_lists(out, 1)
    assert [t[0].tolist() for t in tops] == [[4], [2], [], []] and tops[1][1].tolist() == [6.0]
    # ties come back in label order, NaN is left out
    tl, tf = maxsim_lists_ref.top_lists([(np.array([5, 1, 3, 2]), np.array([1.0, 1.0, nan, 1.0]))], 4)[0]
    assert tl.tolist() == [1, 2, 5] and tf.tolist() == [1.0, 1.0, 1.0]
    assert [d.tolist() for d in maxsim_lists_ref.default_weights([1, 4])] == [[1.0], [0.25] * 4]
