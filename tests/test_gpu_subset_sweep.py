"""GPU: tau sweeps over a subset -- ArrowSpace.search_subset_taus / score_items_taus / search_batch_subset_taus /
score_items_batch_taus.  List j (entry [i][j]) is what the single-tau form returns for taus[j]: each is checked against the
oracle's (or numpy's fp64) score of every item restricted to the subset, at the project's RTOL / atol_for(d), and against the
single-tau calls at 1e-12 relative (lambda_q comes from another search call there).  Within one sweep, and between a sweep and
the score form of the same route, scores are compared bit for bit."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import assert_hits_match, calibrate_eps, calibrate_feature_eps, clustered
from test_gpu_subset import RTOL, atol_for, expected, np_scores, same_as_single, subsets_of

pytestmark = pytest.mark.gpu

TAUS = (1.0, 0.62, 0.0, 0.62, 1.5)   # a duplicate and a tau outside [0, 1]


def draw_queries(aspace, gl, X, rng, b):
    """b perturbed items with lambda_q != 0, their lambda_q; more than 2 b draws fail the test."""
    n, d = X.shape
    Q, lqs, draws = [], [], 0
    while len(Q) < b:
        draws += 1
        assert draws <= 2 * b, f"more than {2 * b} draws for {b} queries with a non-zero lambda_q"
        q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        lq = aspace.query_lambda(q, gl)
        if lq != 0.0:
            Q.append(q)
            lqs.append(lq)
    return np.ascontiguousarray(np.stack(Q)), np.array(lqs)


def id_list(ids):
    ids = np.asarray(ids)
    return np.flatnonzero(ids) if ids.dtype == np.bool_ else ids


def check_sweeps(aspace, gl, Q, taus, subset, ids, scores, topk, d, singles=2):
    """All four forms against scores[i][j], the reference score of every item for query i and taus[j].  The single forms run
    for the first `singles` queries.  Returns the batched lists."""
    ids = id_list(ids)
    uniq = np.unique(ids)
    kk = min(topk, len(uniq))
    b, nt = len(Q), len(taus)

    def check_lists(lists, i):
        assert len(lists) == nt
        for j, hits in enumerate(lists):
            assert len(hits) == kk
            assert_hits_match(hits, expected(scores[i][j], ids, topk), scores[i][j], rtol=RTOL, atol=atol_for(d))

    batched = aspace.search_batch_subset_taus(Q, gl, taus, subset)
    assert len(batched) == b
    rows = aspace.score_items_batch_taus(Q, gl, taus, ids)
    assert rows.shape == (b, nt, len(ids)) and rows.dtype == np.float64
    for i in range(b):
        check_lists(batched[i], i)
        for j in range(nt):
            np.testing.assert_allclose(rows[i, j], scores[i][j][ids], rtol=RTOL, atol=atol_for(d))
    for i in range(min(singles, b)):
        q = np.ascontiguousarray(Q[i])
        check_lists(aspace.search_subset_taus(q, gl, taus, subset), i)
        one = aspace.score_items_taus(q, gl, taus, ids)
        assert one.shape == (nt, len(ids)) and one.dtype == np.float64
        for j in range(nt):
            np.testing.assert_allclose(one[j], scores[i][j][ids], rtol=RTOL, atol=atol_for(d))
    return batched


def raw_sweep(asp, aspace, gl, q, taus, sub, kk):
    t = np.ascontiguousarray(taus, dtype=np.float64)
    nt = len(t)
    idx = np.full((max(nt, 1), max(kk, 1)), -1, dtype=np.int64)
    sc = np.full((max(nt, 1), max(kk, 1)), np.nan)
    ln = np.full(max(nt, 1), -1, dtype=np.int64)
    lq = C.c_double(-1.0)
    st = asp._L.as_search_subset_taus(aspace._h, gl._h, q.ctypes.data, q.shape[0], t.ctypes.data, nt, sub._h, idx.ctypes.data, sc.ctypes.data,
                                      ln.ctypes.data, C.byref(lq))
    flat_i, flat_s = idx.reshape(-1), sc.reshape(-1)
    lists = [list(zip(flat_i[j * kk:j * kk + max(ln[j], 0)].tolist(), flat_s[j * kk:j * kk + max(ln[j], 0)].tolist())) for j in range(nt)]
    return st, lists, lq.value, ln


def raw_batch_sweep(asp, aspace, gl, Q, taus, sub, kk):
    t = np.ascontiguousarray(taus, dtype=np.float64)
    b, nt = Q.shape[0], len(t)
    idx = np.full(max(b * nt * kk, 1), -1, dtype=np.int64)
    sc = np.full(max(b * nt * kk, 1), np.nan)
    ln = np.full(max(b * nt, 1), -1, dtype=np.int64)
    lq = np.full(b, -1.0)
    stt = np.full(b, -7, dtype=np.int32)
    st = asp._L.as_search_subset_batch_taus(aspace._h, gl._h, Q.ctypes.data, b, Q.shape[1], t.ctypes.data, nt, sub._h, idx.ctypes.data,
                                            sc.ctypes.data, ln.ctypes.data, lq.ctypes.data, stt.ctypes.data)
    lists = [[list(zip(idx[p * kk:p * kk + max(ln[p], 0)].tolist(), sc[p * kk:p * kk + max(ln[p], 0)].tolist()))
              for p in range(i * nt, (i + 1) * nt)] for i in range(b)]
    return st, lists, lq, stt, ln.reshape(-1)[:b * nt].reshape(b, nt)


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
@pytest.mark.parametrize("n,d,k,topk,metric,kernel", [(1200, 48, 10, 10, "l2", "gaussian"), (3000, 96, 25, 10, "cosine", "rational")])
def test_sweeps_match_oracle(oracle_lib, n, d, k, topk, metric, kernel, f32):
    """The data, subsets and queries of test_subset_matches_oracle, seed 7 as there: with the CPU oracle alone, all three
    queries of each of the four cases have a non-zero lambda_q under that seed (as under 8 .. 11), so every case checks three."""
    import pyarrowspace_amd as asp
    X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
    if f32:
        X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
    gp = {"eps": calibrate_eps(X, k, metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    ref = oracle_lib.OracleIndex(X, gp)
    rng = np.random.default_rng(7)
    subs = subsets_of(n, rng)
    prepared = {name: aspace.subset(ids) for name, ids in subs}
    Q, sc = [], []
    for _ in range(3):
        q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        try:
            _, lq = ref.search(q, 1.0)
        except oracle_lib.ZeroLambda:
            with pytest.raises(asp.PanicException):
                aspace.search_subset_taus(q, gl, TAUS, prepared["half"])
            with pytest.raises(asp.PanicException):
                aspace.score_items_batch_taus(q[None], gl, TAUS, [0, 1])
            continue
        Q.append(q)
        sc.append([ref.scores(q, tau, lq) for tau in TAUS])
    assert len(Q) >= 2
    Q = np.ascontiguousarray(np.stack(Q))
    for name, ids in subs:
        check_sweeps(aspace, gl, Q, TAUS, prepared[name], ids, sc, topk, d, singles=3)
    # the ad-hoc forms: an array, a list, a mask
    check_sweeps(aspace, gl, Q, TAUS, subs[5][1], subs[5][1], sc, topk, d, singles=1)
    check_sweeps(aspace, gl, Q, TAUS, subs[4][1].tolist(), subs[4][1], sc, topk, d, singles=1)
    check_sweeps(aspace, gl, Q, TAUS, subs[6][1], subs[6][1], sc, topk, d, singles=1)


# ---------------------------------------------------------------- 2. the single-tau calls
@pytest.fixture(scope="module")
def tiles():
    """n = 4000, d = 40, 70 queries with their lambda_q, the items' lambdas."""
    import pyarrowspace_amd as asp
    n, d = 4000, 40
    X = clustered(n, d, nclust=32, seed=20)
    gp = {"eps": calibrate_eps(X, 10), "k": 10, "topk": 10, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(41)
    Q, lqs = draw_queries(aspace, gl, X, rng, 70)
    return X, aspace, gl, Q, lqs, aspace.lambdas()


def ref_scores(X, lam, lqs, Q, taus):
    return [[np_scores(X, lam, lq, q, tau) for tau in taus] for q, lq in zip(Q, lqs)]


@pytest.mark.parametrize("m", [1500, 700])   # the radix select, the sort alone
def test_sweeps_agree_with_the_single_tau_calls(tiles, m):
    import pyarrowspace_amd as asp
    X, aspace, gl, Q, _, _ = tiles
    rng = np.random.default_rng(42)
    ids = rng.choice(4000, m, replace=False)
    sub = aspace.subset(ids)
    Qb = np.ascontiguousarray(Q[:6])
    batched = aspace.search_batch_subset_taus(Qb, gl, TAUS, sub)
    per_tau = [aspace.search_batch_subset(Qb, gl, tau, sub) for tau in TAUS]
    flat = np.array(sorted({i for lists in batched for hits in lists for i, _ in hits}), dtype=np.int64)
    at = {int(i): p for p, i in enumerate(flat)}
    rows_b = aspace.score_items_batch_taus(Qb, gl, TAUS, flat)
    st, _, lq_b, stt, _ = raw_batch_sweep(asp, aspace, gl, Qb, TAUS, sub, 10)
    assert st == 0 and not stt.any()
    for i in range(6):
        q = np.ascontiguousarray(Qb[i])
        st, lists, lq, ln = raw_sweep(asp, aspace, gl, q, TAUS, sub, 10)
        assert st == 0 and ln.tolist() == [10] * 5
        assert lists == aspace.search_subset_taus(q, gl, TAUS, sub) == aspace.search_subset_taus(q, gl, TAUS, ids)
        assert lists[1] == lists[3] and batched[i][1] == batched[i][3]   # the duplicate 0.62
        # lambda_q does not depend on tau; the single calls' searches may sum it on another path
        assert abs(lq_b[i] - lq) <= 1e-12 * abs(lq)
        rows = aspace.score_items_taus(q, gl, TAUS, flat)
        for j, tau in enumerate(TAUS):
            single = aspace.search_subset(q, gl, tau, sub)
            same_as_single(lists[j], single)
            same_as_single(batched[i][j], per_tau[j][i])
            same_as_single(batched[i][j], single)
            idx = np.empty(10, dtype=np.int64)
            sc = np.empty(10)
            ln1, lq1 = C.c_int64(0), C.c_double(0.0)
            assert asp._L.as_search_subset(aspace._h, gl._h, q.ctypes.data, 40, tau, sub._h, idx.ctypes.data, sc.ctypes.data, C.byref(ln1),
                                           C.byref(lq1)) == 0
            assert abs(lq1.value - lq) <= 1e-12 * abs(lq)
            # the score forms return the bits of the lists of their route
            assert [rows[j, at[i_]] for i_, _ in lists[j]] == [s for _, s in lists[j]]
            assert [rows_b[i, j, at[i_]] for i_, _ in batched[i][j]] == [s for _, s in batched[i][j]]
            np.testing.assert_allclose(rows[j], aspace.score_items(q, gl, tau, flat), rtol=1e-12, atol=0.0)
    for j, tau in enumerate(TAUS):
        np.testing.assert_allclose(rows_b[:, j], aspace.score_items_batch(Qb, gl, tau, flat), rtol=1e-12, atol=0.0)


# ---------------------------------------------------------------- 3. tile and group edges
EDGE_M = [1, 3, 4, 5, 127, 128, 129, 1024, 1025]   # the single kernel's four rows a wave, the batched kernel's 128-row tile, the sort's 1024
EDGE_B = [1, 17, 63, 64, 65]                       # the batched kernel's 64-query tile
EDGE_T = [1, 2, 3, 8, 9, 17]                       # groups of up to 8 taus


@pytest.mark.parametrize("m,b,t", [(m, 17, 3) for m in EDGE_M] + [(m, b, 3) for m in (129, 1025) for b in EDGE_B if b != 17] +
                         [(m, 3, t) for m in (5, 1025) for t in EDGE_T if t != 3])
def test_tile_and_group_edges(tiles, m, b, t):
    X, aspace, gl, Q, lqs, lam = tiles
    taus = np.linspace(1.0, 0.0, t) if t > 1 else np.array([0.62])
    ids = np.random.default_rng(1000 + m).choice(4000, m, replace=False)
    check_sweeps(aspace, gl, np.ascontiguousarray(Q[:b]), taus, aspace.subset(ids), ids, ref_scores(X, lam, lqs[:b], Q[:b], taus), 10, 40)


@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
@pytest.mark.parametrize("d", [1, 3, 31, 33, 100, 4100])
def test_feature_count_edges(d, f32):
    """d = 4100 (n = 300): dp > 4096, the query does not fit the LDS staging and the single-query sweep reads it from global memory."""
    import pyarrowspace_amd as asp
    n, b, m = (300, 5, 200) if d > 4096 else (900, 9, 200)
    X = clustered(n, d, nclust=8, seed=300 + d, normalise=d > 1)
    if d == 1:
        X = X + 3.0
    if f32:
        X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 7, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(32)
    Q, lqs = draw_queries(aspace, gl, X, rng, b)
    ids = rng.choice(n, m, replace=False)
    check_sweeps(aspace, gl, Q, TAUS, ids, ids, ref_scores(X, aspace.lambdas(), lqs, Q, TAUS), 7, d)


# ---------------------------------------------------------------- 4. counters
def test_counters(tiles):
    _, aspace, gl, Q, _, _ = tiles
    sub = aspace.subset(np.random.default_rng(43).choice(4000, 500, replace=False))
    ids = sub.ids()
    q, Qb = np.ascontiguousarray(Q[0]), np.ascontiguousarray(Q[:5])
    keys = ("calls", "score_launches", "tau_planes", "lambda_steps")

    def added(f):
        c0 = aspace.subset_sweep_counters()
        f()
        c1 = aspace.subset_sweep_counters()
        assert tuple(c0) == keys
        return [c1[k] - c0[k] for k in keys]

    four, nine = [1.0, 0.62, 0.0, 0.62], np.linspace(0.0, 1.0, 9)
    for f in (lambda t: aspace.search_subset_taus(q, gl, t, sub), lambda t: aspace.score_items_taus(q, gl, t, ids),
              lambda t: aspace.search_batch_subset_taus(Qb, gl, t, sub), lambda t: aspace.score_items_batch_taus(Qb, gl, t, ids)):
        assert added(lambda: f(four)) == [1, 1, 3, 1]
        assert added(lambda: f(nine)) == [1, 2, 9, 1]
        assert added(lambda: f([])) == [0, 0, 0, 0]
    assert added(lambda: aspace.search_subset_taus(q, gl, four, [])) == [1, 0, 0, 1]   # the lambda_q step still runs
    for f in (lambda: aspace.search_subset(q, gl, 0.62, sub), lambda: aspace.score_items(q, gl, 0.62, ids),
              lambda: aspace.search_batch_subset(Qb, gl, 0.62, sub), lambda: aspace.score_items_batch(Qb, gl, 0.62, ids),
              lambda: aspace.search_taus(q, gl, four), lambda: aspace.search_batch_taus(Qb, gl, four)):
        assert added(f) == [0, 0, 0, 0]


# ---------------------------------------------------------------- 5. the chunk budget
def test_the_budget_changes_no_bit(tiles):
    """The default budget: the five planes of all 70 queries in one launch.  1 MiB holds one plane of 43 queries of 3000 items:
    groups of one tau, chunks of one tile of 64 queries -- B = 70 runs two chunks of five groups each."""
    import pyarrowspace_amd as asp
    X, aspace, gl, Q, lqs, lam = tiles
    taus = [1.0, 0.8, 0.62, 0.2, 0.0]
    ids = np.random.default_rng(44).choice(4000, 3000, replace=False)
    sub = aspace.subset(ids)
    Qb = np.ascontiguousarray(Q[:70])
    sc = ref_scores(X, lam, lqs[:70], Qb, taus)
    c0 = aspace.subset_sweep_counters()
    whole = check_sweeps(aspace, gl, Qb, taus, sub, ids, sc, 10, 40, singles=0)
    whole_sc = aspace.score_items_batch_taus(Qb, gl, taus, ids)
    c1 = aspace.subset_sweep_counters()
    assert c1["score_launches"] - c0["score_launches"] == 3 and c1["tau_planes"] - c0["tau_planes"] == 3 * 5   # three calls
    try:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 1) == 0
        assert aspace.search_batch_subset_taus(Qb, gl, taus, sub) == whole
        assert aspace.search_batch_subset_taus(Qb, gl, taus, aspace.subset(ids)) == whole   # buffers made under the small budget
        assert np.array_equal(aspace.score_items_batch_taus(Qb, gl, taus, ids), whole_sc)
        c2 = aspace.subset_sweep_counters()
        assert c2["score_launches"] - c1["score_launches"] == 3 * 2 * 5 and c2["tau_planes"] - c1["tau_planes"] == 3 * 2 * 5
    finally:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 256) == 0
    assert aspace.search_batch_subset_taus(Qb, gl, taus, sub) == whole


# ---------------------------------------------------------------- 6. exact ties
def test_exact_ties_come_back_in_index_order_for_every_tau():
    """The 200 half-scaled copies of row 20 (test_gpu_subset.py) in a subset of more than 1024 ids: at tau = 1 they tie bit for
    bit at the top and straddle the top-k boundary.  For every tau of the sweep the list is the order by (score descending,
    index ascending) of the scores the score form of the same route returns: bit-equal scores come back in index order."""
    import pyarrowspace_amd as asp
    n, d = 4000, 32
    X = clustered(n, d, nclust=16, seed=22)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}   # (before the copies: their distances are 0)
    X[1000:1200] = 0.5 * X[20]
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    q = np.ascontiguousarray(X[20] * 1.01)
    assert aspace.query_lambda(q, gl) != 0.0
    other, _ = draw_queries(aspace, gl, X, np.random.default_rng(35), 2)
    Q = np.ascontiguousarray(np.stack([q, other[0], q, other[1], q]))
    taus = [1.0, 0.62, 0.0, 1.0, 2.0]
    for ids, top in ((np.arange(n), [20, 1000, 1001, 1002, 1003]), (np.arange(n - 1, 499, -1), [1000, 1001, 1002, 1003, 1004])):
        sub = aspace.subset(ids)
        assert sub.size > 1024
        single = aspace.search_subset_taus(q, gl, taus, sub)
        rows = aspace.score_items_taus(q, gl, taus, np.arange(n))
        batched = aspace.search_batch_subset_taus(Q, gl, taus, sub)
        rows_b = aspace.score_items_batch_taus(Q, gl, taus, np.arange(n))
        assert batched[0] == batched[2] == batched[4]
        for j in range(len(taus)):
            assert single[j] == expected(rows[j], ids, 5)
            for i in range(5):
                assert batched[i][j] == expected(rows_b[i, j], ids, 5)
        for lists in (single, batched[0]):
            for j in (0, 3):
                assert [i for i, _ in lists[j]] == top
                assert len({s for _, s in lists[j]}) == 1


# ---------------------------------------------------------------- 7. errors and edges
def test_errors_and_edges():
    import pyarrowspace_amd as asp
    n, d = 800, 32
    X = clustered(n, d, nclust=8, seed=4)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    other, gl2 = asp.ArrowSpaceBuilder.build(gp, X[:400].copy())
    good, _ = draw_queries(aspace, gl, X, np.random.default_rng(38), 3)
    near = np.ascontiguousarray(good[0])
    far = np.full(d, 50.0)   # no item within eps: lambda_q == 0
    Q = np.ascontiguousarray(np.vstack([good[:2], far[None], good[2:]]))
    sub = aspace.subset([1, 2, 3, 700, 40])
    empty = aspace.subset([])
    taus = [1.0, 0.62, 1.0]
    # a NaN or infinite tau anywhere in the list: an error, nothing launched, nothing written
    c0 = aspace.subset_sweep_counters()
    for bad in ([0.5, float("nan")], [float("inf"), 0.5], [0.5, 0.5, -float("inf")]):
        with pytest.raises(ValueError, match="tau"):
            aspace.search_subset_taus(near, gl, bad, sub)
        with pytest.raises(ValueError, match="tau"):
            aspace.score_items_taus(near, gl, bad, [1, 2])
        with pytest.raises(ValueError, match="tau"):
            aspace.search_batch_subset_taus(good, gl, bad, sub)
        with pytest.raises(ValueError, match="tau"):
            aspace.score_items_batch_taus(good, gl, bad, [1, 2])
    out = np.full((2, 2), -5.0)
    badt = np.array([0.5, np.nan])
    ids2 = np.array([3, 1], dtype=np.int64)
    lqc = C.c_double(-1.0)
    assert asp._L.as_score_items_taus(aspace._h, gl._h, near.ctypes.data, d, badt.ctypes.data, 2, ids2.ctypes.data, 2, out.ctypes.data,
                                      C.byref(lqc)) == asp._lib.AS_EINVAL
    assert (out == -5.0).all() and lqc.value == -1.0
    assert aspace.subset_sweep_counters() == c0
    # no taus
    assert aspace.search_subset_taus(near, gl, [], sub) == []
    assert aspace.score_items_taus(near, gl, [], [1, 2, 2]).shape == (0, 3)
    assert aspace.search_batch_subset_taus(good, gl, [], sub) == [[], [], []]
    assert aspace.score_items_batch_taus(good, gl, [], [1, 2, 2]).shape == (3, 0, 3)
    assert aspace.search_subset_taus(far, gl, [], sub) == []   # (nothing runs: no lambda_q step either)
    # the empty subset: empty lists, and the lambda_q step still runs
    for s in (empty, [], np.zeros(n, dtype=bool)):
        assert aspace.search_subset_taus(near, gl, taus, s) == [[], [], []]
        assert aspace.search_batch_subset_taus(good, gl, taus, s) == [[[], [], []]] * 3
    assert aspace.score_items_taus(near, gl, taus, []).shape == (3, 0)
    assert aspace.score_items_batch_taus(good, gl, taus, []).shape == (3, 3, 0)
    for s in (sub, empty, [], [4, 5]):
        with pytest.raises(asp.PanicException):
            aspace.search_subset_taus(far, gl, taus, s)
        with pytest.raises(asp.PanicException):
            aspace.search_batch_subset_taus(Q, gl, taus, s)
    for ids in ([1, 2], []):
        with pytest.raises(asp.PanicException):
            aspace.score_items_taus(far, gl, taus, ids)
        with pytest.raises(asp.PanicException):
            aspace.score_items_batch_taus(Q, gl, taus, ids)
    # a far query among good ones, through the C ABI: its status and lengths, its score rows untouched, the others served
    st, lists, lq, stt, ln = raw_batch_sweep(asp, aspace, gl, Q, taus, sub, 5)
    assert st == 0 and stt.tolist() == [0, 0, asp._lib.AS_EZEROLAMBDA, 0] and lq[2] == 0.0
    assert ln.tolist() == [[5, 5, 5], [5, 5, 5], [0, 0, 0], [5, 5, 5]]
    for i in (0, 1, 3):
        for j, tau in enumerate(taus):
            same_as_single(lists[i][j], aspace.search_subset(np.ascontiguousarray(Q[i]), gl, tau, sub))
    st, lists, lq, stt, ln = raw_batch_sweep(asp, aspace, gl, Q, taus, empty, 0)
    assert st == 0 and stt.tolist() == [0, 0, asp._lib.AS_EZEROLAMBDA, 0] and not ln.any()
    out = np.full((4, 3, 2), -5.0)
    t3 = np.array(taus)
    lq4, st4 = np.zeros(4), np.zeros(4, dtype=np.int32)
    assert asp._L.as_score_items_batch_taus(aspace._h, gl._h, Q.ctypes.data, 4, d, t3.ctypes.data, 3, ids2.ctypes.data, 2, out.ctypes.data,
                                            lq4.ctypes.data, st4.ctypes.data) == 0
    assert st4.tolist() == [0, 0, asp._lib.AS_EZEROLAMBDA, 0] and (out[2] == -5.0).all()
    for i in (0, 1, 3):
        assert np.array_equal(out[i, 0], out[i, 2])
        for j, tau in enumerate(taus):
            np.testing.assert_allclose(out[i, j], aspace.score_items(np.ascontiguousarray(Q[i]), gl, tau, ids2), rtol=1e-12, atol=0.0)
    # the single-tau forms' errors
    with pytest.raises(ValueError, match="another space"):
        other.search_subset_taus(np.ascontiguousarray(X[3] * 1.01), gl2, taus, sub)
    with pytest.raises(ValueError, match="another space"):
        other.search_batch_subset_taus(np.ascontiguousarray(good), gl2, taus, sub)
    with pytest.raises(ValueError, match="query length"):
        aspace.search_subset_taus(np.ascontiguousarray(near[:10]), gl, taus, sub)
    with pytest.raises(ValueError, match="query length"):
        aspace.score_items_taus(np.ascontiguousarray(near[:10]), gl, taus, [1, 2])
    with pytest.raises(ValueError, match="query length"):
        aspace.search_batch_subset_taus(np.ascontiguousarray(good[:, :10]), gl, taus, sub)
    with pytest.raises(ValueError, match="query length"):
        aspace.score_items_batch_taus(np.ascontiguousarray(good[:, :10]), gl, taus, [1, 2])
    for bad in ([0, n], [-1, 3]):
        with pytest.raises(ValueError):
            aspace.search_subset_taus(near, gl, taus, bad)
        with pytest.raises(ValueError, match="id"):
            aspace.score_items_taus(near, gl, taus, bad)
        with pytest.raises(ValueError):
            aspace.search_batch_subset_taus(good, gl, taus, bad)
        with pytest.raises(ValueError, match="id"):
            aspace.score_items_batch_taus(good, gl, taus, bad)
    with pytest.raises(TypeError):
        aspace.search_subset_taus(near, None, taus, sub)
    with pytest.raises(TypeError):
        aspace.search_subset_taus(near, gl, [[1.0]], sub)
    with pytest.raises(TypeError):
        aspace.search_batch_subset_taus(good[0], gl, taus, sub)
    # B == 0
    none = np.empty((0, d))
    assert aspace.search_batch_subset_taus(none, gl, taus, sub) == []
    assert aspace.score_items_batch_taus(none, gl, taus, [1, 2, 2]).shape == (0, 3, 3)


@pytest.mark.parametrize("extra", [{"lambda_mode": "feature", "metric": "cosine", "kernel": "rational"}, {"force_exact": True}],
                         ids=["feature", "force_exact"])
def test_feature_lambda_and_force_exact_indexes(extra):
    import pyarrowspace_amd as asp
    n, d = 800, 24
    X = clustered(n, d, nclust=8, seed=18)
    eps = calibrate_feature_eps(X, 6) if "lambda_mode" in extra else calibrate_eps(X, 6)
    aspace, gl = asp.ArrowSpaceBuilder.build(dict({"eps": eps, "k": 6, "topk": 8, "p": 2.0, "sigma": None}, **extra), X)
    rng = np.random.default_rng(19)
    ids = rng.choice(n, 200, replace=False)
    Q, lqs = draw_queries(aspace, gl, X, rng, 4)
    batched = check_sweeps(aspace, gl, Q, TAUS, ids, ids, ref_scores(X, aspace.lambdas(), lqs, Q, TAUS), 8, d, singles=4)
    for j, tau in enumerate(TAUS):
        per_tau = aspace.search_batch_subset(Q, gl, tau, ids)
        for i in range(4):
            q = np.ascontiguousarray(Q[i])
            same_as_single(batched[i][j], per_tau[i])
            same_as_single(aspace.search_subset_taus(q, gl, TAUS, ids)[j], aspace.search_subset(q, gl, tau, ids))


# ---------------------------------------------------------------- 8. threads
def test_sweeps_and_single_calls_on_one_handle_from_several_threads(tiles):
    _, aspace, gl, Q, _, _ = tiles
    ids = np.random.default_rng(45).choice(4000, 1500, replace=False)
    sub = aspace.subset(ids)
    Qb = np.ascontiguousarray(Q[:12])
    taus = [1.0, 0.62, 0.0]
    batched = aspace.search_batch_subset_taus(Qb, gl, taus, sub)
    sweeps = [aspace.search_subset_taus(q, gl, taus, sub) for q in Qb]
    singles = [aspace.search_subset(q, gl, 0.62, sub) for q in Qb]
    errors = []

    def run(f):
        def body():
            try:
                for _ in range(3):
                    f()
            except BaseException as e:   # noqa: BLE001
                errors.append(e)
        return threading.Thread(target=body)

    def f_batched():
        assert aspace.search_batch_subset_taus(Qb, gl, taus, sub) == batched

    def f_sweep():
        assert [aspace.search_subset_taus(q, gl, taus, sub) for q in Qb] == sweeps

    def f_single():
        assert [aspace.search_subset(q, gl, 0.62, sub) for q in Qb] == singles

    th = [run(f_batched), run(f_sweep), run(f_single)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]


# ---------------------------------------------------------------- 9. many blocks
def test_many_blocks():
    """20 000 ids: 157 row tiles of the batched kernel, and more groups of four rows than the single kernel's grid has waves (its
    grid-stride loop takes a second trip); B = 70: two query tiles."""
    import pyarrowspace_amd as asp
    n, d, b = 20_000, 32, 70
    X = clustered(n, d, nclust=64, seed=12)
    gp = {"eps": calibrate_eps(X, 4), "k": 4, "topk": 3, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    Q, lqs = draw_queries(aspace, gl, X, np.random.default_rng(13), b)
    taus = [1.0, 0.62, 0.3, 0.0]
    ids = np.arange(n)
    check_sweeps(aspace, gl, Q, taus, aspace.subset(ids), ids, ref_scores(X, aspace.lambdas(), lqs, Q, taus), 3, d)
