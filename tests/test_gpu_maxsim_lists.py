"""GPU: late-interaction re-ranking of per-need candidate documents -- ArrowSpace.search_maxsim_lists /
score_maxsim_lists: B needs of J_b query vectors, each need with its own candidate groups, scored by one ragged launch that reads
a candidate row once per tile of the need's vectors, then folded and selected on the device.  Every expected value is the numpy
reference tests/maxsim_lists_ref.py over the bits `score_lists_batch` writes for the call's flattened vectors, each vector with its
need's expanded id list; labels and score bits must be equal, no tolerance (NaN is compared as NaN, not by payload).  Indexes and
query recipe: tests/test_gpu_maxsim.py's, more vectors by tests/test_gpu_maxsim_batch.py's `vectors`."""
import ctypes as C
import threading

import numpy as np
import pytest

import fused_ref
import maxsim_lists_ref as ref
from conftest import assert_hits_match, calibrate_eps, clustered
from test_gpu_maxsim import SHAPES, TAU, bits, index, same_scores, weights_of
from test_gpu_maxsim_batch import vectors

pytestmark = pytest.mark.gpu


def tuning(asp, key, value):
    assert asp._L.as_set_tuning(key, value) == 0


def counted(aspace, call):
    c0 = aspace.maxsim_lists_counters()
    out = call()
    c1 = aspace.maxsim_lists_counters()
    return out, {k: c1[k] - c0[k] for k in c1}


def lists_scores(asp, aspace, gl, V, id_lists, tau=TAU):
    """What `score_lists_batch` writes for the vectors V, vector v with the id list id_lists[v], through the C entry (the Python
    method panics where a lambda_q is 0; the entry leaves that vector's scores unwritten and reports it) -> (one float64 array
    per vector, NaN where nothing was written; served flags)."""
    V = np.ascontiguousarray(V, dtype=np.float64)
    offs = np.zeros(len(id_lists) + 1, dtype=np.int64)
    np.cumsum([len(l) for l in id_lists], out=offs[1:])
    ids = np.ascontiguousarray(np.concatenate(id_lists) if len(id_lists) else np.empty(0), dtype=np.int64)
    out = np.full(max(len(ids), 1), np.nan)
    stt = np.zeros(V.shape[0], dtype=np.int32)
    st = asp._L.as_score_lists_batch(aspace._h, gl._h, V.ctypes.data_as(C.c_void_p), V.shape[0], V.shape[1], float(tau),
                                     ids.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None,
                                     stt.ctypes.data_as(C.c_void_p))
    assert st == 0, asp._lib.last_error()
    return [out[offs[v]:offs[v + 1]] for v in range(V.shape[0])], (stt != asp._lib.AS_EZEROLAMBDA).tolist()


def expected(asp, aspace, gl, needs, labels, lists, wper, tau=TAU):
    """(per need (labels, F) by the reference, the served flags per need, the entries per need)."""
    V = np.concatenate(needs)
    ids = [ref.members(labels, l) for l in lists]
    rows, served = lists_scores(asp, aspace, gl, V, [ids[b] for b, Q in enumerate(needs) for _ in range(len(Q))], tau)
    S, sv, o = [], [], 0
    for b, Q in enumerate(needs):
        S.append(np.stack(rows[o:o + len(Q)]).reshape(len(Q), len(ids[b])))
        sv.append(served[o:o + len(Q)])
        o += len(Q)
    return ref.maxsim_lists(S, [labels[i] for i in ids], wper, sv), sv, ids


def check_both_forms(asp, aspace, gl, needs, labels, grp, lists, passed, wper, ng, tau=TAU, **kw):
    """`score_maxsim_lists` and `search_maxsim_lists` against the reference -> (scores, hits, the reference's per-need (labels, F))."""
    want, sv, ids = expected(asp, aspace, gl, needs, labels, lists, wper, tau)
    got = aspace.score_maxsim_lists(needs, gl, tau, grp, lists, weights=passed, **kw)
    assert len(got) == len(needs)
    for b, (lab, F) in enumerate(want):
        l = np.asarray(lists[b], dtype=np.int64)
        assert got[b].dtype == np.float64 and got[b].shape == l.shape, b
        same_scores(got[b], F[np.searchsorted(lab, l)] if len(l) else np.empty(0))   # the caller's order, duplicates kept
    hits = aspace.search_maxsim_lists(needs, gl, tau, grp, ng, lists, weights=passed, **kw)
    assert len(hits) == len(needs)
    for b, (wl, wf) in enumerate(ref.top_lists(want, ng)):
        assert len(hits[b]) == min(ng, int((~np.isnan(want[b][1])).sum())), b
        assert [l for l, _ in hits[b]] == wl.tolist(), b
        assert bits([v for _, v in hits[b]]) == bits(wf), b
    return got, hits, want


def cut(V, Js):
    """Needs of Js vectors each, taken from V one after the other, starting over when V runs out (needs may share vectors)."""
    needs, o = [], 0
    for J in Js:
        if o + J > len(V):
            o = 0
        needs.append(np.ascontiguousarray(V[o:o + J]))
        o += J
    return needs


def need_weights(Js, which, rng):
    """0: the default, 1: random signed weights, 2: random with one weight of 0 -> (what the caller passes, per-need weights)."""
    if which == 0:
        return None, ref.default_weights(Js)
    per = []
    for J in Js:
        w = rng.uniform(-1.0, 1.0, J)
        if which == 2:
            w[J // 2] = 0.0
        per.append(w)
    return per, per


def label_recipes(n, rng):
    """name -> (labels, documents a need names)."""
    wide = np.concatenate([[-2 ** 62, -5, 2 ** 40 + 3, 2 ** 62], rng.choice(10 ** 6, 33, replace=False)])   # large and negative labels
    return {"groups of 10": (np.arange(n) // 10, 12), "singletons": (np.arange(n), 150), "one for all": (np.full(n, 42), 1),
            "171 interleaved": (np.arange(n) % 171 - 40, 9), "wide values": (wide[rng.integers(0, 37, n)], 5)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_bits_of_both_forms(name):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    geo = aspace.maxsim_lists_geometry()
    T, R = geo["tile"], geo["segment"]
    assert T == min(32, 4096 // (-(-X.shape[1] // 32) * 32)) and R == 64
    V = vectors(name)
    rng = np.random.default_rng(1800)
    turn = 0
    for lname, (labels, ndoc) in label_recipes(n, rng).items():
        grp = aspace.groups(labels)
        every = np.unique(labels)
        for Js in ((1, 2, T - 1, T, T + 1, 2 * T + 1), (1, 2, 5, T, T + 1, 3, 1)):
            needs = cut(V, Js)
            lists = [rng.choice(every, min(ndoc, len(every)), replace=False) for _ in Js]
            passed, wper = need_weights(Js, turn % 3, rng)
            (_, hits, want), dc = counted(aspace, lambda: check_both_forms(asp, aspace, gl, needs, labels, grp, lists, passed, wper,
                                                                           (10, 1024, 1)[turn % 3]))
            turn += 1
            E = [int(np.isin(labels, l).sum()) for l in lists]
            assert (dc["calls"], dc["needs"], dc["lambda_steps"]) == (2, 2 * len(Js), 2), lname
            assert dc["vectors_served"] == 2 * sum(Js) and dc["score_launches"] == dc["fold_launches"] == 2
            assert dc["pairs"] == 2 * sum(e * J for e, J in zip(E, Js))
            assert dc["row_reads"] == 2 * sum(e * -(-J // T) for e, J in zip(E, Js))   # a row once per tile, not once per vector


def test_segment_edges():
    """Documents of 1, R - 1, R, R + 1 and 3 R + 5 members; expanded lists that end exactly on a segment edge and one past it; a
    need that covers every document; one document shared by all needs."""
    name = "1200x48"
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    geo = aspace.maxsim_lists_geometry()
    T, R = geo["tile"], geo["segment"]
    sizes = [1, R - 1, R, R + 1, 3 * R + 5]
    labels = np.empty(n, dtype=np.int64)
    o = 0
    for g, m in enumerate(sizes):
        labels[o:o + m] = g
        o += m
    labels[o:] = 5 + (np.arange(n - o) // 10)
    perm = np.random.default_rng(5).permutation(n)   # the members of a document are not neighbours in memory
    labels = labels[perm]
    grp = aspace.groups(labels)
    every = np.unique(labels)
    lists = [[0, 1], [0, 2], [0, 1, 2], [0, 3], every, [0, 4], [0, 1, 2, 3], [0]]
    E = [int(np.isin(labels, l).sum()) for l in lists]
    assert E[:4] == [R, R + 1, 2 * R, R + 2] and E[4] == n and E[6] == 3 * R + 1 and E[7] == 1
    Js = (1, 3, T + 1, 2, 4, T, 2 * T + 1, 5)
    needs = cut(vectors(name), Js)
    rng = np.random.default_rng(1801)
    for which in range(3):
        passed, wper = need_weights(Js, which, rng)
        check_both_forms(asp, aspace, gl, needs, labels, grp, lists, passed, wper, (1024, 3, 1)[which])


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_callers_order_duplicates_empty_lists_and_arrays(name):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    labels = np.arange(n) // 10
    grp = aspace.groups(labels)
    rng = np.random.default_rng(1802)
    Js = (3, 2, 4)
    needs = cut(vectors(name), Js)
    base = [rng.choice(n // 10, 40, replace=False) for _ in Js]
    plain = aspace.search_maxsim_lists(needs, gl, TAU, grp, 1024, [np.sort(l) for l in base])
    scores = aspace.score_maxsim_lists(needs, gl, TAU, grp, [np.sort(l) for l in base])
    mixed = [np.concatenate([rng.permutation(l), l[:7], l[:3]]) for l in base]   # permuted, duplicates added
    assert aspace.search_maxsim_lists(needs, gl, TAU, grp, 1024, mixed) == plain
    got = aspace.score_maxsim_lists(needs, gl, TAU, grp, mixed)
    for b in range(3):
        at = dict(zip(np.sort(base[b]).tolist(), bits(scores[b])))
        assert bits(got[b]) == [at[l] for l in mixed[b].tolist()]
        assert sorted(l for l, _ in plain[b]) == np.sort(base[b]).tolist()
    # an empty list between two served needs; lists as tuples and arrays of other integer types
    lists = [base[0].astype(np.int32), [], tuple(int(l) for l in base[2])]
    (got, hits, _), dc = counted(aspace, lambda: check_both_forms(asp, aspace, gl, needs, labels, grp, lists, None, ref.default_weights(Js), 10))
    assert hits[1] == [] and got[1].shape == (0,) and len(hits[0]) == len(hits[2]) == 10
    assert dc["lambda_steps"] == 2 and dc["vectors_served"] == 2 * (3 + 4)   # the empty need's vectors are scored against nothing
    # every list empty: nothing is launched, the lambda_q step runs
    (hits, dc) = counted(aspace, lambda: aspace.search_maxsim_lists(needs, gl, TAU, grp, 5, [[], [], []]))
    assert hits == [[], [], []] and dc["score_launches"] == 0 and dc["lambda_steps"] == 1
    assert [a.shape for a in aspace.score_maxsim_lists(needs, gl, TAU, grp, [[], [], []])] == [(0,)] * 3
    # a (B, C) integer array gives a (B, C) array
    arr = np.stack([l[:16] for l in mixed])
    got = aspace.score_maxsim_lists(needs, gl, TAU, grp, arr)
    assert isinstance(got, np.ndarray) and got.shape == (3, 16) and got.dtype == np.float64
    rows = aspace.score_maxsim_lists(needs, gl, TAU, grp, [r for r in arr])
    assert bits(got) == bits(np.stack(rows))
    assert aspace.search_maxsim_lists(needs, gl, TAU, grp, 4, arr) == aspace.search_maxsim_lists(needs, gl, TAU, grp, 4, [r for r in arr])


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_against_the_batched_form_over_the_same_members(name):
    """(a): default weights, every need given all groups: 1e-12 relative against `score_maxsim_batch` (the batched forms sum in
    another order), the search lists equal except inside such ties."""
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    labels = np.arange(n) // 10
    grp = aspace.groups(labels)
    every = np.unique(labels)
    Js = (1, 4, 9)
    needs = cut(vectors(name), Js)
    got = aspace.score_maxsim_lists(needs, gl, TAU, grp, [every] * 3)
    want = aspace.score_maxsim_batch(needs, gl, TAU, grp, every)
    np.testing.assert_allclose(np.stack(got), want, rtol=1e-12, atol=0.0)
    hits = aspace.search_maxsim_lists(needs, gl, TAU, grp, 10, [every] * 3)
    batch = aspace.search_maxsim_batch(needs, gl, TAU, grp, 10)
    for b in range(3):
        assert_hits_match(hits[b], batch[b], all_scores=dict(zip(every.tolist(), want[b].tolist())), rtol=1e-12)


@pytest.mark.parametrize("name", list(SHAPES))
def test_b_and_c_one_vector_and_singleton_groups(name):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    V = vectors(name)
    rng = np.random.default_rng(1803)
    # (b) J_b = 1 and weight 1.0: F(g) is the maximum of `score_lists_batch`'s scores over g's members, bit for bit
    labels = np.arange(n) % 171
    grp = aspace.groups(labels)
    lists = [np.sort(rng.choice(171, 20, replace=False)) for _ in range(4)]
    ids = [ref.members(labels, l) for l in lists]
    rows = aspace.score_lists_batch(V[:4], gl, TAU, ids)
    got = aspace.score_maxsim_lists([V[b:b + 1] for b in range(4)], gl, TAU, grp, lists, weights=[[1.0]] * 4)
    for b in range(4):
        assert bits(got[b]) == bits([rows[b][labels[ids[b]] == g].max() + 0.0 for g in lists[b]])
    # (c) every item its own group: F is the "sum" fold of `score_lists_batch`'s rows
    grp = aspace.groups(np.arange(n))
    Js = (3, 5)
    needs = cut(V, Js)
    lists = [np.sort(rng.choice(n, 130, replace=False)) for _ in Js]
    w = [rng.uniform(-1.0, 1.0, J) for J in Js]
    flat = aspace.score_lists_batch(np.concatenate(needs), gl, TAU, [lists[b] for b, J in enumerate(Js) for _ in range(J)])
    got = aspace.score_maxsim_lists(needs, gl, TAU, grp, lists, weights=w)
    hits = aspace.search_maxsim_lists(needs, gl, TAU, grp, 7, lists, weights=w)
    o = 0
    for b, J in enumerate(Js):
        F = fused_ref.fuse(np.stack(flat[o:o + J]) + 0.0, w[b], "sum")
        o += J
        assert bits(got[b]) == bits(F)
        wi, wf = fused_ref.top(lists[b], F, 7)
        assert [l for l, _ in hits[b]] == wi.tolist() and bits([v for _, v in hits[b]]) == bits(wf)


@pytest.mark.parametrize("name", list(SHAPES))
def test_d_chunks_grid_and_the_order_of_the_needs(name):
    """(d): a one-MiB budget splits the call into several chunks, a small grid cap sends blocks through later loop trips, the needs
    change places: every need keeps its bits (for the same lambda_q: the reference is taken under the same arrangement)."""
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    T = aspace.maxsim_lists_geometry()["tile"]
    labels = np.arange(n) // 10
    grp = aspace.groups(labels)
    every = np.unique(labels)
    rng = np.random.default_rng(1804)
    Js = (2 * T + 1, 3, T, 1, T + 1, 7)
    needs = cut(vectors(name), Js)
    lists = [every, rng.choice(every, 30, replace=False), every[::2], rng.choice(every, 5, replace=False), every[5:], every[:50]]
    passed, wper = need_weights(Js, 1, rng)
    (base, hits, _), d0 = counted(aspace, lambda: check_both_forms(asp, aspace, gl, needs, labels, grp, lists, passed, wper, 10))
    assert d0["score_launches"] == 2
    try:
        tuning(asp, b"subset_batch_mib", 1)   # 131072 scores a chunk: the call holds more
        assert sum(J * int(np.isin(labels, l).sum()) for J, l in zip(Js, lists)) > (1 << 20) // 8
        (got, h1, _), d1 = counted(aspace, lambda: check_both_forms(asp, aspace, gl, needs, labels, grp, lists, passed, wper, 10))
        assert d1["score_launches"] >= 2 * 2 and d1["fold_launches"] == d1["score_launches"] and d1["lambda_steps"] == 2
        assert (d1["pairs"], d1["row_reads"]) == (d0["pairs"], d0["row_reads"])
        assert h1 == hits and all(bits(a) == bits(b) for a, b in zip(got, base))
        tuning(asp, b"filtered_grid_cap", 3)
        got, h2, _ = check_both_forms(asp, aspace, gl, needs, labels, grp, lists, passed, wper, 10)
        assert h2 == hits and all(bits(a) == bits(b) for a, b in zip(got, base))
    finally:
        tuning(asp, b"subset_batch_mib", 256)
        tuning(asp, b"filtered_grid_cap", 0)
    try:
        tuning(asp, b"filtered_grid_cap", 2)
        got, h3, _ = check_both_forms(asp, aspace, gl, needs, labels, grp, lists, passed, wper, 10)
        assert h3 == hits and all(bits(a) == bits(b) for a, b in zip(got, base))
    finally:
        tuning(asp, b"filtered_grid_cap", 0)
    order = [3, 0, 5, 2, 4, 1]
    check_both_forms(asp, aspace, gl, [needs[i] for i in order], labels, grp, [lists[i] for i in order],
                     [passed[i] for i in order], [wper[i] for i in order], 10)
    # the other needs' lists do not matter: need 1 beside other lists
    others = [every[:3], lists[1], every[:1], [], every[:2], every[:4]]
    alone = aspace.score_maxsim_lists(needs, gl, TAU, grp, others, weights=passed)
    assert bits(alone[1]) == bits(base[1])


def test_ties_come_back_in_label_order():
    import pyarrowspace_amd as asp
    n, d = 1000, 40
    X = clustered(n, d, nclust=8, seed=6)   # tests/test_gpu_maxsim.py's recipe: three identical rows
    X[500] = X[10]
    X[900] = X[10]
    gp = {"eps": calibrate_eps(X, 8), "k": 8, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    q, r = np.ascontiguousarray(X[10] * 1.01), np.ascontiguousarray(X[10] * 0.99)
    needs = [np.stack([q, r]), q[None, :], np.stack([r, q, r])]
    weights = [[0.25, 0.75], None, [0.5, 0.25, 0.125]]
    wper = [np.array([0.25, 0.75]), np.array([1.0]), np.array([0.5, 0.25, 0.125])]
    for a, b, c in ((7, 3, 5), (3, 5, 7), (2 ** 40, -6, 0)):
        labels = np.arange(n) + 100
        labels[10], labels[500], labels[900] = a, b, c
        lists = [[c, 150, a, b, 170], [b, a, c], [160, b, c, a]]
        for ng in (3, 2):   # the whole tie; the cut inside the tie
            _, hits, want = check_both_forms(asp, aspace, gl, needs, labels, labels, lists, weights, wper, ng, tau=1.0)
            for y in range(3):
                lab, F = want[y]
                assert bits(F[np.searchsorted(lab, [a, b, c])]) == bits([F[np.searchsorted(lab, a)]] * 3)   # equal bits: a tie
                assert [l for l, _ in hits[y]] == sorted((a, b, c))[:ng]


def test_non_finite_items():
    """tests/test_gpu_filtered_nonfinite.py's fixture: an item with an inf joins no maximum; a document whose members all score
    NaN is left out of the search form and scores NaN.  768 features: tiles of 5 vectors, a row one column chunk."""
    import test_gpu_filtered_nonfinite as nf
    asp, fx, gp, aspace, gl, V, _ = nf.index("700x768f32")
    n = fx["X"].shape[0]
    T = aspace.maxsim_lists_geometry()["tile"]
    assert T == 5
    rng = np.random.default_rng(1805)
    Js = (1, 2, T - 1, T, T + 1, 2 * T + 1)
    needs = cut(V, Js)
    for lname in ("crafted", "singletons"):
        labels = nf.grouped_labels(fx)[lname]
        grp = aspace.groups(labels)
        every = np.unique(labels)
        lists = [every if b % 2 == 0 else np.concatenate([[labels[fx["nan_rows"][0]], labels[fx["lam_rows"][0]]], rng.choice(every, 40, replace=False)])
                 for b in range(len(Js))]
        for which in (0, 1):
            passed, wper = need_weights(Js, which, rng)
            got, hits, want = check_both_forms(asp, aspace, gl, needs, labels, grp, lists, passed, wper, 1024)
            for y, (lab, F) in enumerate(want):
                assert not set(l for l, _ in hits[y]) & set(lab[np.isnan(F)].tolist())
        if lname == "crafted":   # group 0: the inf run alone; group 1: ten numbers and ten NaN items
            got = aspace.score_maxsim_lists(needs, gl, TAU, grp, [[0, 1]] * len(Js))
            assert all(np.isnan(g[0]) and not np.isnan(g[1]) for g in got)
            hits = aspace.search_maxsim_lists(needs, gl, TAU, grp, 5, [[0, 1]] * len(Js))
            assert all([l for l, _ in h] == [1] for h in hits)
            assert aspace.search_maxsim_lists(needs, gl, TAU, grp, 5, [[0]] * len(Js)) == [[]] * len(Js)


@pytest.mark.parametrize("name", list(SHAPES))
def test_zero_lambda(name):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n, d = X.shape
    V = vectors(name)
    rng = np.random.default_rng(1806)
    far = np.full(d, 50.0)   # no item within eps: lambda_q == 0 (the recipe of tests/test_gpu_maxsim.py::test_zero_lambda)
    labels = np.arange(n) // 10
    grp = aspace.groups(labels)
    # such a vector first, in the middle and last in a need; a need made only of such vectors between ordinary needs
    needs = [V[50:53], np.stack([far, V[53], V[54]]), np.stack([V[55], far * 1.5, V[56]]), np.stack([far, far * 1.5]), V[57:59],
             np.stack([V[59], V[60], far])]
    Js = [len(Q) for Q in needs]
    lists = [rng.choice(n // 10, 25, replace=False) for _ in needs]
    weights = [None, [0.5, -0.25, 0.75], [0.4, 0.3, -0.2], None, [2.0, 1.0], None]
    wper = [np.full(3, 1.0 / 3), np.array([0.5, -0.25, 0.75]), np.array([0.4, 0.3, -0.2]), np.full(2, 0.5), np.array([2.0, 1.0]), np.full(3, 1.0 / 3)]
    launched = ("vectors_served", "score_launches", "row_reads", "pairs", "fold_launches")
    # raise: the panic of the whole call with nothing gathered: the counters do not move past the lambda_q step
    for call in (lambda: aspace.search_maxsim_lists(needs, gl, TAU, grp, 10, lists, weights=weights),
                 lambda: aspace.score_maxsim_lists(needs, gl, TAU, grp, lists, weights=weights)):
        c0 = aspace.maxsim_lists_counters()
        with pytest.raises(asp.PanicException):
            call()
        c1 = aspace.maxsim_lists_counters()
        assert (c1["calls"] - c0["calls"], c1["needs"] - c0["needs"], c1["lambda_steps"] - c0["lambda_steps"]) == (1, 6, 1)
        assert all(c1[k] == c0[k] for k in launched)
    # skip: the served vectors of each need with their own weights, not renormalised; need 3 has none left
    want, sv, _ = expected(asp, aspace, gl, needs, labels, lists, wper)
    assert sv == [[True] * 3, [False, True, True], [True, False, True], [False, False], [True, True], [True, True, False]]
    (got, hits, _), dc = counted(aspace, lambda: check_both_forms(asp, aspace, gl, needs, labels, grp, lists, weights, wper, 10,
                                                                  on_zero_lambda="skip"))
    assert hits[3] == [] and np.isnan(got[3]).all() and got[3].shape == (25,)
    assert all(len(hits[b]) == 10 and not np.isnan(got[b]).any() for b in (0, 1, 2, 4, 5))
    assert dc["vectors_served"] == 2 * 11 and dc["score_launches"] == 2 and dc["lambda_steps"] == 2
    E = [int(np.isin(labels, l).sum()) for l in lists]
    assert dc["pairs"] == 2 * sum(e * sum(s) for e, s in zip(E, sv)) and dc["row_reads"] == 2 * sum(e for e, s in zip(E, sv) if any(s))
    # no vector of any need served: B empty lists / NaN under skip, nothing launched; the panic under raise
    none = [np.stack([far, far * 1.5]), far[None, :]]
    out, dc = counted(aspace, lambda: aspace.search_maxsim_lists(none, gl, TAU, grp, 3, lists[:2], on_zero_lambda="skip"))
    assert out == [[], []] and all(dc[k] == 0 for k in launched) and dc["lambda_steps"] == 1
    out = aspace.score_maxsim_lists(none, gl, TAU, grp, lists[:2], on_zero_lambda="skip")
    assert [o.shape for o in out] == [(25,), (25,)] and all(np.isnan(o).all() for o in out)
    with pytest.raises(asp.PanicException):
        aspace.search_maxsim_lists(none, gl, TAU, grp, 3, lists[:2])


@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
@pytest.mark.parametrize("d", [1, 3, 31, 33, 100, 800, 4100])
def test_feature_count_edges(d, f32):
    """tests/test_gpu_lists.py::test_feature_count_edges' recipe on fp32 items and on an fp64 (force_exact) index.  d = 800: a row
    is more than one column chunk and the tile still sits in LDS; d = 4100: one vector does not fit the staging and is read from
    global memory."""
    import pyarrowspace_amd as asp
    from test_gpu_lists import draw_queries
    n, nv = (300, 5) if d > 4096 else (900, 12)
    X = clustered(n, d, nclust=8, seed=300 + d, normalise=d > 1)
    if d == 1:
        X = X + 3.0
    if f32:
        X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 7, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    T = aspace.maxsim_lists_geometry()["tile"]
    dp = -(-d // 32) * 32
    assert T == (min(32, 4096 // dp) if dp <= 4096 else 1)
    rng = np.random.default_rng(33)
    Q, _ = draw_queries(aspace, gl, X, rng, nv)
    Js = (2, 1, 2) if d > 4096 else (T + 1 if T < 6 else 6, 1, 5)
    needs = cut(np.ascontiguousarray(Q), Js)
    labels = np.arange(n) % 97
    grp = aspace.groups(labels)
    lists = [rng.choice(97, m, replace=False) for m in (20, 97, 1)]
    for which in (0, 1):
        passed, wper = need_weights(Js, which, rng)
        check_both_forms(asp, aspace, gl, needs, labels, grp, lists, passed, wper, 7)


def test_errors_on_the_device_path():
    asp, X, gp, aspace, gl, _, _ = index("1200x48")
    n, d = X.shape
    V = vectors("1200x48")
    other, gl2 = asp.ArrowSpaceBuilder.build(gp, X[:400].copy())
    needs = [V[:3], V[3:5]]
    grp = aspace.groups(np.arange(n) // 7)
    lists = [[0, 1], [2]]
    wide = [np.ascontiguousarray(np.concatenate([Q, np.ones((len(Q), 1))], axis=1)) for Q in needs]
    cases = ((ValueError, "label 172 is not one of the groups", lambda: aspace.search_maxsim_lists(needs, gl, TAU, grp, 3, [[0, 172], [2]])),
             (ValueError, "label -1 is not one of the groups", lambda: aspace.score_maxsim_lists(needs, gl, TAU, grp, [[0], [-1]])),
             (TypeError, "integer group labels", lambda: aspace.search_maxsim_lists(needs, gl, TAU, grp, 3, [[0.0], [2.0]])),
             (TypeError, "integer group labels", lambda: aspace.score_maxsim_lists(needs, gl, TAU, grp, [[True], [False]])),
             (ValueError, "3 label lists for 2 needs", lambda: aspace.search_maxsim_lists(needs, gl, TAU, grp, 3, [[0], [1], [2]])),
             (ValueError, "n_groups", lambda: aspace.search_maxsim_lists(needs, gl, TAU, grp, 0, lists)),
             (ValueError, "n_groups", lambda: aspace.search_maxsim_lists(needs, gl, TAU, grp, 1025, lists)),
             (ValueError, "another space", lambda: other.search_maxsim_lists(needs, gl2, TAU, grp, 3, lists)),
             (ValueError, "another space", lambda: other.score_maxsim_lists(needs, gl2, TAU, grp, lists)),
             (ValueError, "labels", lambda: aspace.search_maxsim_lists(needs, gl, TAU, np.arange(n - 1), 3, lists)),
             (ValueError, "query length", lambda: aspace.search_maxsim_lists(wide, gl, TAU, grp, 3, lists)))
    for exc, match, call in cases:
        c0, o0 = aspace.maxsim_lists_counters(), other.maxsim_lists_counters()
        with pytest.raises(exc, match=match):
            call()
        assert aspace.maxsim_lists_counters() == c0 and other.maxsim_lists_counters() == o0   # nothing launched, no lambda_q step
    # the C ABI's own refusals behind the handles: documents that are not their group's members
    Vc, offs = np.ascontiguousarray(np.concatenate(needs)), np.array([0, 3, 5], dtype=np.int64)
    lab, sc, ln = np.full(6, 7, dtype=np.int64), np.full(6, 5.0), np.full(2, 9, dtype=np.int64)
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    good = (i64([0, 1, 2]), i64([0, 2]), i64([0, 7, 14]), i64(list(range(7)) + list(range(14, 21))))
    bad = (("need_docs", (i64([1, 1, 2]),) + good[1:]), ("need_docs must not decrease", (i64([0, 2, 1]),) + good[1:]),
           ("not one of the groups", (good[0], i64([0, 999]), good[2], good[3])),
           ("increase strictly", (i64([0, 2, 2]), i64([2, 0]), good[2], good[3])),
           ("holds 6 entries", (good[0], good[1], i64([0, 6, 13]), good[3])),
           ("not the next member", (good[0], good[1], good[2], i64(list(range(7)) + list(range(7, 14))))),
           ("not the next member", (good[0], good[1], good[2], i64([1, 0, 2, 3, 4, 5, 6] + list(range(14, 21))))),
           ("not the next member", (good[0], good[1], good[2], i64([0, 1, 2, 3, 4, 5, n] + list(range(14, 21))))))
    for what, (nd, dl, df, ids) in bad:
        c0 = aspace.maxsim_lists_counters()
        ln[:] = 9
        rc = asp._L.as_search_maxsim_lists(aspace._h, gl._h, Vc.ctypes.data, offs.ctypes.data, 2, 5, d, TAU, None, 0, grp._h, 3, nd.ctypes.data,
                                           dl.ctypes.data, df.ctypes.data, ids.ctypes.data, lab.ctypes.data, sc.ctypes.data, ln.ctypes.data,
                                           None, None)
        assert rc == asp._lib.AS_EINVAL and what in asp._lib.last_error(), (what, asp._lib.last_error())
        assert ln.tolist() == [0, 0] and lab.tolist() == [7] * 6 and sc.tolist() == [5.0] * 6
        rc = asp._L.as_score_maxsim_lists(aspace._h, gl._h, Vc.ctypes.data, offs.ctypes.data, 2, 5, d, TAU, None, 0, grp._h, nd.ctypes.data,
                                          dl.ctypes.data, df.ctypes.data, ids.ctypes.data, sc.ctypes.data, None, None)
        assert rc == asp._lib.AS_EINVAL and what in asp._lib.last_error() and sc.tolist() == [5.0] * 6
        assert aspace.maxsim_lists_counters() == c0
    nd, dl, df, ids = good
    rc = asp._L.as_search_maxsim_lists(aspace._h, gl._h, Vc.ctypes.data, offs.ctypes.data, 2, 5, d, TAU, None, 0, grp._h, 3, nd.ctypes.data,
                                       dl.ctypes.data, df.ctypes.data, ids.ctypes.data, lab.ctypes.data, sc.ctypes.data, ln.ctypes.data, None, None)
    assert rc == 0 and ln.tolist() == [1, 1] and lab[0] == 0 and lab[3] == 2
    assert [(int(lab[0]), float(sc[0]))] == aspace.search_maxsim_lists(needs, gl, TAU, grp, 3, [[0], [2]])[0]


def test_a_shard_of_a_row_sharded_index_is_not_supported():
    """A 200-row shard at row offset 200 of 600 items (tests/test_gpu_maxsim_batch.py's way to make one): AS_EUNSUPPORTED from both
    entries, nothing written but the lengths."""
    import torch

    import pyarrowspace_amd as asp
    from pyarrowspace_amd.dist import HipEngine
    n, d, k, lo, hi = 600, 32, 5, 200, 400
    X = clustered(n, d, nclust=4, seed=9)
    gp = {"eps": calibrate_eps(X, k), "k": k, "topk": 5, "p": 2.0, "sigma": None}
    whole = HipEngine(gp)
    whole.create_space(torch.from_numpy(X).cuda())
    idx, dist, gy, cnt = whole.knn_rows(0, n)
    valid = torch.arange(k, device=idx.device)[None, :] < cnt[:, None].long()
    src = torch.arange(n, device=idx.device)[:, None].expand(n, k)[valid]
    tgt, ed, eg = idx[valid].long(), dist[valid], gy[valid]
    here = (tgt >= lo) & (tgt < hi)
    e = HipEngine(gp)
    e.create_space(torch.from_numpy(X[lo:hi].copy()).cuda())
    e.graph_shard_csr(n, lo, idx[lo:hi].contiguous(), dist[lo:hi].contiguous(), gy[lo:hi].contiguous(), cnt[lo:hi].contiguous(),
                      (tgt[here] - lo).int(), src[here].int(), ed[here], eg[here])
    assert int(e.L.as_graph_row_offset(e.gr)) == lo and int(e.L.as_graph_ncols(e.gr)) == n
    labels = np.ascontiguousarray(np.arange(hi - lo) // 10, dtype=np.int64)
    grp = C.c_void_p()
    assert e.L.as_groups_create(e.sp, labels.ctypes.data, hi - lo, C.byref(grp)) == 0
    Vc, offs = np.ascontiguousarray(X[lo:lo + 5]), np.array([0, 3, 5], dtype=np.int64)
    lab, sc, ln = np.full(6, 7, dtype=np.int64), np.full(6, 5.0), np.full(2, 9, dtype=np.int64)
    lq, st = np.full(5, 3.0), np.full(2, 9, dtype=np.int32)
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    nd, dl, df, ids = i64([0, 1, 2]), i64([0, 2]), i64([0, 10, 20]), i64(list(range(10)) + list(range(20, 30)))
    try:
        rc = e.L.as_search_maxsim_lists(e.sp, e.gr, Vc.ctypes.data, offs.ctypes.data, 2, 5, d, TAU, None, 0, grp, 3, nd.ctypes.data, dl.ctypes.data,
                                        df.ctypes.data, ids.ctypes.data, lab.ctypes.data, sc.ctypes.data, ln.ctypes.data, lq.ctypes.data,
                                        st.ctypes.data)
        assert rc == asp._lib.AS_EUNSUPPORTED and "row-sharded" in asp._lib.last_error() and ln.tolist() == [0, 0]
        rc = e.L.as_score_maxsim_lists(e.sp, e.gr, Vc.ctypes.data, offs.ctypes.data, 2, 5, d, TAU, None, 0, grp, nd.ctypes.data, dl.ctypes.data,
                                       df.ctypes.data, ids.ctypes.data, sc.ctypes.data, lq.ctypes.data, st.ctypes.data)
        assert rc == asp._lib.AS_EUNSUPPORTED and "row-sharded" in asp._lib.last_error()
        assert lab.tolist() == [7] * 6 and sc.tolist() == [5.0] * 6 and lq.tolist() == [3.0] * 5 and st.tolist() == [9, 9]
        out = (C.c_int64 * 9)()
        assert e.L.as_maxsim_lists_counters(e.sp, out, 9) == 0 and list(out)[:8] == [0] * 8
    finally:
        e.L.as_groups_free(grp)
        e.close()
        whole.close()


def test_two_threads_on_one_space():
    asp, X, gp, aspace, gl, _, _ = index("1200x48")
    n = X.shape[0]
    labels = np.arange(n) // 10
    grp = aspace.groups(labels)
    grp._members()
    rng = np.random.default_rng(1807)
    V = vectors("1200x48")
    jobs = []
    for t in range(2):
        Js = (3, 1, 6) if t == 0 else (2, 9)
        needs = cut(V[20 * t:], Js)
        lists = [rng.choice(n // 10, 30, replace=False) for _ in Js]
        jobs.append((needs, lists))
    want = [(aspace.search_maxsim_lists(nd, gl, TAU, grp, 10, ls), aspace.score_maxsim_lists(nd, gl, TAU, grp, ls)) for nd, ls in jobs]
    got, errors = [None, None], []

    def work(t):
        try:
            nd, ls = jobs[t]
            for _ in range(5):
                got[t] = (aspace.search_maxsim_lists(nd, gl, TAU, grp, 10, ls), aspace.score_maxsim_lists(nd, gl, TAU, grp, ls))
        except BaseException as exc:   # noqa: BLE001 (reported below)
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        assert got[t][0] == want[t][0]
        assert all(bits(a) == bits(b) for a, b in zip(got[t][1], want[t][1]))
