"""GPU: grouped search -- ArrowSpace.search_grouped / search_batch_grouped: the best items of the best groups,
picked on the device.  Every expected value is the numpy reference tests/grouped_ref.py over the bits `score_items` (single form)
or `score_items_batch` (batched form) returns for the same ids -- the route there was before; labels, indices and score bits
must be equal, no tolerance.  Those two score forms are themselves held against the fp64 oracle by tests/test_gpu_subset.py and
tests/test_gpu_subset_batch.py, so no further oracle comparison is made here.  Shapes and index recipe: tests/test_gpu_fused.py's."""
import numpy as np
import pytest

import grouped_ref
from conftest import calibrate_eps, clustered

pytestmark = pytest.mark.gpu

TAU = 0.62
# (n, d, k, topk, metric, kernel, rounded through float32)
SHAPES = {"1200x48": (1200, 48, 10, 10, "l2", "gaussian", False), "1500x51": (1500, 51, 8, 6, "l2", "gaussian", False),
          "700x768f32": (700, 768, 12, 15, "l2", "gaussian", True), "3000x96cos": (3000, 96, 25, 10, "cosine", "rational", False)}
NVEC = 66   # served query vectors kept per shape: one past the batched score kernel's query tile, and one more
_built = {}


def index(name):
    """One index per shape for the whole module: (asp, X, graph parameters, aspace, gl, NVEC query vectors whose lambda_q is
    not 0)."""
    if name not in _built:
        import pyarrowspace_amd as asp
        n, d, k, topk, metric, kernel, f32 = SHAPES[name]
        X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
        if f32:
            X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
        gp = {"eps": calibrate_eps(X, k, metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
        aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
        rng = np.random.default_rng(n)
        vecs = []
        while len(vecs) < NVEC:
            q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
            if aspace.query_lambda(q, gl) != 0.0:
                vecs.append(q)
        _built[name] = (asp, X, gp, aspace, gl, np.stack(vecs))
    return _built[name]


def label_recipes(n, rng):
    pool = np.concatenate([[-5, 2 ** 40 + 3], rng.choice(10 ** 6, 35, replace=False)])   # 37 labels, one negative, one above 2^40
    skew = np.arange(n, dtype=np.int64) + 10
    skew[rng.random(n) < 0.9] = 7
    return {"singletons": np.arange(n), "one for all": np.full(n, 42), "i // 7": np.arange(n) // 7,
            "37 random": pool[rng.integers(0, 37, n)], "skew": skew}


def without_some_groups(labels, rng):
    """Ids of a subset that leaves whole groups out: every third distinct label is dropped (a single label: half the items)."""
    u = np.unique(labels)
    if len(u) == 1:
        return np.sort(rng.choice(len(labels), len(labels) // 2, replace=False))
    return np.flatnonzero(~np.isin(labels, u[::3]))


def same(got, want):
    """Equal labels, indices and score bits."""
    flat = lambda r: [(int(l), [(int(i), int(np.float64(s).view(np.uint64))) for i, s in mem]) for l, mem in r]
    assert flat(got) == flat(want)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("name", list(SHAPES))
def test_bits_against_the_route_there_was_before(name):
    asp, X, gp, aspace, gl, V = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(100)
    q = V[3]
    every = np.arange(n)
    s_all = aspace.score_items(q, gl, TAU, every)
    assert not np.isnan(s_all).any()
    fixed = [("none", None, None), ("257 ids", np.sort(rng.choice(n, 257, replace=False)), None), ("one id", np.array([int(rng.integers(0, n))]), None)]
    fixed = [(sname, ids, None if ids is None else aspace.subset(ids)) for sname, ids, _ in fixed]
    for lname, labels in label_recipes(n, rng).items():
        grp = aspace.groups(labels)
        assert grp.ngroups == len(grp) == len(np.unique(labels)) and grp.labels().tolist() == labels.tolist()
        part = without_some_groups(labels, rng)
        for sname, ids, handle in fixed + [("whole groups out", part, aspace.subset(part))]:
            ids = every if ids is None else ids
            for ng in (1, 5, 1024):
                for pg in (1, 2, 16):
                    got = aspace.search_grouped(q, gl, TAU, grp, ng, pg, subset=handle)
                    same(got, grouped_ref.grouped(ids, labels[ids], s_all[ids], ng, pg))
            if sname == "whole groups out":   # a group whose every item lies outside the subset never appears
                assert not set(l for l, _ in got) & set(labels.tolist()) - set(labels[ids].tolist())
        # ad-hoc labels and an ad-hoc subset give the prepared handles' answer
        want = aspace.search_grouped(q, gl, TAU, grp, 5, 2, subset=fixed[1][2])
        assert aspace.search_grouped(q, gl, TAU, labels.tolist(), 5, 2, subset=fixed[1][1][::-1].copy()) == want


@pytest.mark.parametrize("name", list(SHAPES))
def test_consequences_of_s14(name):
    asp, X, gp, aspace, gl, V = index(name)
    n, topk = X.shape[0], gp["topk"]
    rng = np.random.default_rng(101)
    some = np.sort(rng.choice(n, 257, replace=False))
    q = V[7]
    single, one = aspace.groups(np.arange(n)), aspace.groups(np.full(n, -9))
    for ids in (np.arange(n), some):
        sub = aspace.subset(ids)
        hits = aspace.search_subset(q, gl, TAU, sub)
        assert len(hits) == topk
        # every item its own group, per_group = 1: the heads are search_subset's list, bit for bit, for every n_groups <= topk
        for ng in (1, topk - 1, topk):
            got = aspace.search_grouped(q, gl, TAU, single, ng, 1, subset=sub)
            assert [l for l, _ in got] == [i for i, _ in hits[:ng]]
            assert [mem[0][0] for _, mem in got] == [i for i, _ in hits[:ng]] and all(len(mem) == 1 for _, mem in got)
            assert bits([mem[0][1] for _, mem in got]) == bits([v for _, v in hits[:ng]])
        # one label for all: the single group's members are the first per_group entries of that list
        for pg in (1, 2, min(topk, 16)):
            got = aspace.search_grouped(q, gl, TAU, one, 3, pg, subset=sub)
            assert len(got) == 1 and got[0][0] == -9
            assert [i for i, _ in got[0][1]] == [i for i, _ in hits[:pg]] and bits([v for _, v in got[0][1]]) == bits([v for _, v in hits[:pg]])
    # over-asking: per_group beyond a group returns the whole group, n_groups beyond the groups returns them all
    labels = np.arange(n) // 7
    got = aspace.search_grouped(q, gl, TAU, labels, 1024, 16)
    assert len(got) == min(len(np.unique(labels)), 1024)
    sizes = np.bincount(labels)
    assert all(len(mem) == sizes[l] for l, mem in got)
    got = aspace.search_grouped(q, gl, TAU, labels, 1024, 16, subset=some)
    assert sorted(l for l, _ in got) == np.unique(labels[some]).tolist()
    assert sorted(i for _, mem in got for i, _ in mem) == some.tolist()


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("name", ["1500x51", "3000x96cos"])
def test_batched(name, B):
    asp, X, gp, aspace, gl, V = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(102)
    Q = V[:B]
    some = np.sort(rng.choice(n, 257, replace=False))
    sub = aspace.subset(some)
    recipes = label_recipes(n, rng)
    S = aspace.score_items_batch(Q, gl, TAU, np.arange(n))
    assert not np.isnan(S).any()
    answers = []
    for budget in (256, 1):   # one MiB: several chunks of 64 queries where B = 65
        try:
            assert asp._L.as_set_tuning(b"subset_batch_mib", budget) == 0
            got = []
            for lname in ("i // 7", "37 random"):
                labels = recipes[lname]
                grp = aspace.groups(labels)
                for ids, handle in ((np.arange(n), None), (some, sub)):
                    for ng, pg in ((5, 1), (3, 3), (1024, 16)):
                        res = aspace.search_batch_grouped(Q, gl, TAU, grp, ng, pg, subset=handle)
                        assert len(res) == B
                        for i in range(B):
                            same(res[i], grouped_ref.grouped(ids, labels[ids], S[i][ids], ng, pg))
                        got.append(res)
            answers.append(got)
        finally:
            assert asp._L.as_set_tuning(b"subset_batch_mib", 256) == 0
    assert answers[0] == answers[1]   # results never depend on the budget
    assert aspace.search_batch_grouped(Q[:0], gl, TAU, recipes["i // 7"], 5) == []


def test_ties():
    import pyarrowspace_amd as asp
    n, d = 1000, 40
    X = clustered(n, d, nclust=8, seed=6)
    X[500] = X[10]
    X[900] = X[10]
    gp = {"eps": calibrate_eps(X, 8), "k": 8, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    q = np.ascontiguousarray(X[10] * 1.01)
    s = aspace.score_items(q, gl, 1.0, [10, 500, 900])
    assert bits(s)[0] == bits(s)[1] == bits(s)[2]   # the precondition: three scores with equal bits
    assert s[0] > np.delete(aspace.score_items(q, gl, 1.0, np.arange(n)), [10, 500, 900]).max()
    sb = aspace.score_items_batch(q[None, :], gl, 1.0, [10, 500, 900])[0]
    assert bits(sb)[0] == bits(sb)[1] == bits(sb)[2]
    forms = ((lambda *a, **k: aspace.search_grouped(q, gl, 1.0, *a, **k), s[0]),
             (lambda *a, **k: aspace.search_batch_grouped(np.stack([q, q]), gl, 1.0, *a, **k)[1], sb[0]))
    for call, top in forms:
        A, B = 5, 3
        labels = np.arange(n) + 100
        labels[[10, 900]] = A
        labels[500] = B
        got = call(labels, 2, 2)
        assert [l for l, _ in got] == [A, B]   # the heads 10 and 500 tie: index order
        assert [i for i, _ in got[0][1]] == [10, 900] and [i for i, _ in got[1][1]] == [500]
        assert bits([v for _, mem in got for _, v in mem]) == bits([top] * 3)
        got = call(labels, 2, 1)
        assert [(l, [i for i, _ in mem]) for l, mem in got] == [(A, [10]), (B, [500])]
        # the labels swapped: the order follows the indices again
        labels[[10, 900]] = B
        labels[500] = A
        got = call(labels, 2, 2)
        assert [(l, [i for i, _ in mem]) for l, mem in got] == [(B, [10, 900]), (A, [500])]
        # all three in one group: index order inside it
        labels[500] = B
        got = call(labels, 1, 16)
        assert [(l, [i for i, _ in mem]) for l, mem in got] == [(B, [10, 500, 900])]
        # a subset without item 10: 500 heads
        got = call(labels, 1, 16, subset=np.arange(11, n))
        assert [(l, [i for i, _ in mem]) for l, mem in got] == [(B, [500, 900])]


def test_no_state_survives_a_call():
    asp, X, gp, aspace, gl, V = index("1500x51")
    n = X.shape[0]
    rng = np.random.default_rng(103)
    q = V[11]
    s_all = aspace.score_items(q, gl, TAU, np.arange(n))
    every = np.arange(n)
    single = aspace.groups(every)
    four = np.arange(n) % 4
    g4 = aspace.groups(four)
    some = np.sort(rng.choice(n, 300, replace=False))
    first = aspace.search_grouped(q, gl, TAU, single, 20, 3)
    same(first, grouped_ref.grouped(every, every, s_all, 20, 3))
    same(aspace.search_grouped(q, gl, TAU, g4, 20, 1), grouped_ref.grouped(every, four, s_all, 20, 1))
    same(aspace.search_grouped(q, gl, TAU, g4, 2, 5, subset=some), grouped_ref.grouped(some, four[some], s_all[some], 2, 5))
    last = aspace.search_grouped(q, gl, TAU, single, 20, 3)
    assert last == first
    # ... and the batched form after them, then the single form once more
    Q = V[:3]
    S = aspace.score_items_batch(Q, gl, TAU, every)
    res = aspace.search_batch_grouped(Q, gl, TAU, g4, 3, 4)
    for i in range(3):
        same(res[i], grouped_ref.grouped(every, four, S[i], 3, 4))
    assert aspace.search_grouped(q, gl, TAU, single, 20, 3) == first


def test_atomics_bound():
    asp, X, gp, aspace, gl, V = index("3000x96cos")
    n = X.shape[0]
    q = V[5]
    s_all = aspace.score_items(q, gl, TAU, np.arange(n))
    for labels, bound in ((np.full(n, 1), 47), (np.arange(n) // 50, 106)):
        changes = int((labels[1:] != labels[:-1]).sum())
        assert -(-n // 64) + changes == bound
        grp = aspace.groups(labels)
        for pg in (1, 3):
            c0 = aspace.grouped_counters()
            got = aspace.search_grouped(q, gl, TAU, grp, 10, pg)
            c1 = aspace.grouped_counters()
            same(got, grouped_ref.grouped(np.arange(n), labels, s_all, 10, pg))
            grown = c1["max_atomics"] - c0["max_atomics"]
            print(f"labels {len(np.unique(labels))} groups, per_group {pg}: {grown} max-atomics, bound {pg * bound}, {n} positions")
            assert 0 < grown <= pg * bound
            assert c1["lambda_steps"] - c0["lambda_steps"] == 1 and c1["calls"] - c0["calls"] == 1
            assert c1["pick_launches"] - c0["pick_launches"] == 2 * pg
            assert c1["scores_examined"] - c0["scores_examined"] == 2 * pg * n
            assert c1["groups"] - c0["groups"] == len(got) and c1["members"] - c0["members"] == sum(len(mem) for _, mem in got)


def test_zero_lambda_and_the_refusals():
    asp, X, gp, aspace, gl, V = index("1200x48")
    n, d = X.shape
    far = np.ascontiguousarray(np.full(d, 50.0))   # no item within eps
    assert aspace.query_lambda(far, gl) == 0.0 and aspace.query_lambda(V[0], gl) != 0.0
    labels = np.arange(n) // 7
    grp = aspace.groups(labels)
    for subset in (None, [1, 2, 3], []):
        c0 = aspace.grouped_counters()
        with pytest.raises(asp.PanicException):
            aspace.search_grouped(far, gl, TAU, grp, 3, 2, subset=subset)
        with pytest.raises(asp.PanicException):
            aspace.search_batch_grouped(np.stack([V[0], far, V[1]]), gl, TAU, grp, 3, 2, subset=subset)
        c1 = aspace.grouped_counters()
        assert c1["lambda_steps"] - c0["lambda_steps"] == 2 and c1["calls"] - c0["calls"] == 2
    # the C ABI serves the other queries of a batch and reports the one in out_status
    import ctypes as C
    Q = np.ascontiguousarray(np.stack([V[0], far, V[1]]))
    S = aspace.score_items_batch(Q[[0, 2]], gl, TAU, np.arange(n))
    lab, cnt = np.zeros((3, 3), dtype=np.int64), np.zeros((3, 3), dtype=np.int64)
    idx, sc = np.zeros((3, 6), dtype=np.int64), np.zeros((3, 6))
    ng, st, lq = np.full(3, 9, dtype=np.int64), np.zeros(3, dtype=np.int32), np.zeros(3)
    assert asp._L.as_search_grouped_batch(aspace._h, gl._h, Q.ctypes.data, 3, d, TAU, grp._h, 3, 2, None, lab.ctypes.data, cnt.ctypes.data,
                                          idx.ctypes.data, sc.ctypes.data, ng.ctypes.data, lq.ctypes.data, st.ctypes.data) == 0
    assert st.tolist() == [0, asp._lib.AS_EZEROLAMBDA, 0] and ng.tolist() == [3, 0, 3] and lq[1] == 0.0 and lq[0] != 0.0
    for row, i in ((0, 0), (1, 2)):
        want = grouped_ref.grouped(np.arange(n), labels, S[row], 3, 2)
        got = [(lab[i, s], list(zip(idx[i].reshape(3, 2)[s][:cnt[i, s]].tolist(), sc[i].reshape(3, 2)[s][:cnt[i, s]].tolist()))) for s in range(3)]
        same(got, want)
    # refusals on the device path: nothing is launched, no lambda_q step either
    other, gl2 = asp.ArrowSpaceBuilder.build(gp, X[:400].copy())
    sub = aspace.subset([1, 2, 3])
    wide = np.ascontiguousarray(np.concatenate([V[0], [1.0]]))
    cases = ((ValueError, "another space", lambda: other.search_grouped(V[0], gl2, TAU, grp, 3)),
             (ValueError, "another space", lambda: other.search_batch_grouped(V[:2], gl2, TAU, grp, 3)),
             (ValueError, "another space", lambda: other.search_grouped(V[0], gl2, TAU, np.arange(400), 3, subset=sub)),
             (ValueError, "query length", lambda: aspace.search_grouped(wide, gl, TAU, grp, 3)),
             (ValueError, "labels", lambda: aspace.search_grouped(V[0], gl, TAU, np.arange(n - 1), 3)),
             (ValueError, "id", lambda: aspace.search_grouped(V[0], gl, TAU, grp, 3, subset=[0, n])))
    for exc, match, call in cases:
        c0, o0 = aspace.grouped_counters(), other.grouped_counters()
        with pytest.raises(exc, match=match):
            call()
        assert aspace.grouped_counters() == c0 and other.grouped_counters() == o0
    for ngv, pgv, what in ((0, 1, "n_groups"), (1025, 1, "n_groups"), (1, 0, "per_group"), (1, 17, "per_group")):
        n1 = C.c_int64(5)
        st1 = asp._L.as_search_grouped(aspace._h, gl._h, V[0].ctypes.data, d, TAU, grp._h, ngv, pgv, None, lab.ctypes.data, cnt.ctypes.data,
                                       idx.ctypes.data, sc.ctypes.data, C.byref(n1), None)
        assert st1 == asp._lib.AS_EINVAL and what in asp._lib.last_error() and n1.value == 0
    # an empty subset: an empty answer, but the lambda_q step runs
    c0 = aspace.grouped_counters()
    assert aspace.search_grouped(V[0], gl, TAU, grp, 3, subset=[]) == []
    assert aspace.search_batch_grouped(V[:2], gl, TAU, grp, 3, subset=[]) == [[], []]
    c1 = aspace.grouped_counters()
    assert c1["lambda_steps"] - c0["lambda_steps"] == 2 and c1["pick_launches"] == c0["pick_launches"]
    # the neighbours on a handle are undisturbed
    before = aspace.search_subset(V[0], gl, TAU, sub)
    aspace.search_grouped(V[0], gl, TAU, grp, 3, 2, subset=sub)
    assert aspace.search_subset(V[0], gl, TAU, sub) == before
