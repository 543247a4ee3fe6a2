"""GPU: batched filtered search -- ArrowSpace.search_batch_subset / score_items_batch.  List i of the batched form is what
`search_subset(items[i], ...)` returns, row i of the batched scores what `score_items(items[i], ...)` returns: each is checked
against the oracle's (or numpy's fp64) score of every item restricted to the subset, at the project's RTOL / atol_for(d), and
against the single form at 1e-12 relative (the two kernels sum in different orders).  Queries: perturbed items whose lambda_q is
not 0, at most 2 B draws for B queries."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import assert_hits_match, calibrate_eps, calibrate_feature_eps, clustered
from test_gpu_subset import RTOL, atol_for, expected, np_scores, same_as_single, subsets_of

pytestmark = pytest.mark.gpu


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


def check_batch(aspace, gl, Q, tau, subset, ids, all_scores, topk, d, single=True):
    """all_scores[i]: the reference score of every item for query i."""
    got = aspace.search_batch_subset(Q, gl, tau, subset)
    assert len(got) == len(Q)
    uniq = set(np.unique(ids).tolist())
    for i, hits in enumerate(got):
        assert len(hits) == min(topk, len(uniq))
        assert all(j in uniq for j, _ in hits)
        assert_hits_match(hits, expected(all_scores[i], ids, topk), all_scores[i], rtol=RTOL, atol=atol_for(d))
        if single:
            same_as_single(hits, aspace.search_subset(Q[i], gl, tau, subset))
    return got


def raw_batch(asp, aspace, gl, Q, tau, sub, kk):
    b = Q.shape[0]
    idx = np.full((b, max(kk, 1)), -1, dtype=np.int64)
    sc = np.full((b, max(kk, 1)), np.nan)
    ln = np.full(b, -1, dtype=np.int64)
    lq = np.full(b, -1.0)
    stt = np.full(b, -7, dtype=np.int32)
    st = asp._L.as_search_subset_batch(aspace._h, gl._h, Q.ctypes.data, b, Q.shape[1], float(tau), sub._h, idx.ctypes.data, sc.ctypes.data,
                                       ln.ctypes.data, lq.ctypes.data, stt.ctypes.data)
    lists = [list(zip(idx[i, :max(ln[i], 0)].tolist(), sc[i, :max(ln[i], 0)].tolist())) for i in range(b)]
    return st, lists, lq, stt, ln


# ---------------------------------------------------------------- 1. the oracle and the single form
@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
@pytest.mark.parametrize("n,d,k,topk,metric,kernel", [(1200, 48, 10, 10, "l2", "gaussian"), (3000, 96, 25, 10, "cosine", "rational"),
                                                       (2000, 768, 25, 15, "l2", "gaussian"), (1500, 51, 8, 6, "l2", "gaussian")])
def test_batch_matches_oracle_and_single(oracle_lib, n, d, k, topk, metric, kernel, f32):
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
    Q, _ = draw_queries(aspace, gl, X, rng, 5)
    lqs = [ref.search(q, 1.0)[1] for q in Q]
    for tau in (1.0, 0.62, 0.0):
        sc = [ref.scores(q, tau, lq) for q, lq in zip(Q, lqs)]
        for name, ids in subs:
            idl = np.flatnonzero(ids) if ids.dtype == np.bool_ else ids
            check_batch(aspace, gl, Q, tau, prepared[name], idl, sc, topk, d)
        # the ad-hoc forms: an array, a list, a mask
        check_batch(aspace, gl, Q, tau, subs[5][1], subs[5][1], sc, topk, d)
        check_batch(aspace, gl, Q, tau, subs[4][1].tolist(), subs[4][1], sc, topk, d)
        check_batch(aspace, gl, Q, tau, subs[6][1], np.flatnonzero(subs[6][1]), sc, topk, d)


# ---------------------------------------------------------------- 2. tile edges
TILE_M = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1024, 1025]
TILE_B = [1, 2, 15, 16, 17, 31, 33, 63, 65, 130]


@pytest.fixture(scope="module")
def tiles():
    """n = 4000, d = 64, 130 queries and numpy's fp64 score of every item for each, computed once."""
    import pyarrowspace_amd as asp
    n, d, tau = 4000, 64, 0.62
    X = clustered(n, d, nclust=32, seed=20)
    gp = {"eps": calibrate_eps(X, 10), "k": 10, "topk": 10, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(31)
    Q, lqs = draw_queries(aspace, gl, X, rng, max(TILE_B))
    lam = aspace.lambdas()
    sc = [np_scores(X, lam, lq, q, tau) for q, lq in zip(Q, lqs)]
    subs = {m: rng.choice(n, m, replace=False) for m in TILE_M}
    return aspace, gl, Q, sc, subs, tau, d


@pytest.mark.parametrize("m,b", [(m, 17) for m in TILE_M] + [(m, b) for m in (129, 1025) for b in TILE_B if b != 17])
def test_tile_edges(tiles, m, b):
    aspace, gl, Q, sc, subs, tau, d = tiles
    ids = subs[m]
    check_batch(aspace, gl, np.ascontiguousarray(Q[:b]), tau, aspace.subset(ids), ids, sc[:b], 10, d)
    got = aspace.score_items_batch(np.ascontiguousarray(Q[:b]), gl, tau, ids)
    assert got.shape == (b, m)
    np.testing.assert_allclose(got, np.stack([s[ids] for s in sc[:b]]), rtol=RTOL, atol=atol_for(d))


# ---------------------------------------------------------------- 3. d edges
@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
@pytest.mark.parametrize("d", [1, 3, 31, 33, 100])
def test_feature_count_edges(d, f32):
    import pyarrowspace_amd as asp
    n, b, m, tau = 900, 9, 200, 0.62
    X = clustered(n, d, nclust=8, seed=300 + d, normalise=d > 1)
    if d == 1:
        X = X + 3.0
    if f32:
        X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 7, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(32)
    Q, lqs = draw_queries(aspace, gl, X, rng, b)
    lam = aspace.lambdas()
    sc = [np_scores(X, lam, lq, q, tau) for q, lq in zip(Q, lqs)]
    ids = rng.choice(n, m, replace=False)
    check_batch(aspace, gl, Q, tau, ids, ids, sc, 7, d)
    np.testing.assert_allclose(aspace.score_items_batch(Q, gl, tau, ids), np.stack([s[ids] for s in sc]), rtol=RTOL, atol=atol_for(d))


# ---------------------------------------------------------------- 4. several chunks
def test_several_chunks_give_the_same_lists(tiles):
    """A budget of 1 MiB holds 43 queries' scores of 3000 items: chunks of one tile of 64 queries, B = 70 runs two, the last short."""
    import pyarrowspace_amd as asp
    aspace, gl, Q, sc, _, tau, d = tiles
    rng = np.random.default_rng(33)
    ids = rng.choice(4000, 3000, replace=False)
    sub = aspace.subset(ids)
    Qb = np.ascontiguousarray(Q[:70])
    whole = check_batch(aspace, gl, Qb, tau, sub, ids, sc[:70], 10, d)
    whole_sc = aspace.score_items_batch(Qb, gl, tau, ids)
    try:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 1) == 0
        assert aspace.search_batch_subset(Qb, gl, tau, sub) == whole
        assert aspace.search_batch_subset(Qb, gl, tau, aspace.subset(ids)) == whole   # buffers made under the small budget
        assert np.array_equal(aspace.score_items_batch(Qb, gl, tau, ids), whole_sc)
    finally:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 256) == 0
    assert aspace.search_batch_subset(Qb, gl, tau, sub) == whole


# ---------------------------------------------------------------- 5. many blocks and rounds of the selection
@pytest.fixture(scope="module")
def big():
    """n = 70 000: more than one block and more than one round of every selection kernel (the recipe of test_gpu_subset.py)."""
    import pyarrowspace_amd as asp
    n, d = 70_000, 32
    X = clustered(n, d, nclust=64, seed=12)
    gp = {"eps": calibrate_eps(X, 4), "k": 4, "topk": 3, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(13)
    Q, lqs = draw_queries(aspace, gl, X, rng, 5)
    return X, aspace, gl, aspace.lambdas(), Q, lqs


@pytest.mark.parametrize("which", ["all", "65537", "duplicates"])
def test_many_blocks_and_rounds(big, which):
    X, aspace, gl, lam, Q, lqs = big
    n, d = X.shape
    rng = np.random.default_rng(14)
    ids = {"all": np.arange(n), "65537": rng.choice(n, 65537, replace=False),
           "duplicates": rng.choice(n, 300, replace=False)[rng.integers(0, 300, 70_000)]}[which]
    sub = aspace.subset(ids)
    assert sub.size == len(np.unique(ids))
    for tau in (1.0, 0.62, 0.0):
        sc = [np_scores(X, lam, lq, q, tau) for q, lq in zip(Q, lqs)]
        check_batch(aspace, gl, Q, tau, sub, ids, sc, 3, d)
        if which == "duplicates":   # the same ids scored one by one, the caller's order and duplicates kept
            np.testing.assert_allclose(aspace.score_items_batch(Q, gl, tau, ids), np.stack([s[ids] for s in sc]), rtol=RTOL, atol=atol_for(d))


# ---------------------------------------------------------------- 6. the full subset is search_batch
@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
def test_full_subset_is_search_batch(f32):
    import pyarrowspace_amd as asp
    n, d, k, topk, b = 2500, 200, 12, 20, 40
    X = clustered(n, d, nclust=24, seed=3)
    if f32:
        X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
    gp = {"eps": calibrate_eps(X, k), "k": k, "topk": topk, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    full = aspace.subset(np.ones(n, dtype=bool))
    Q, _ = draw_queries(aspace, gl, X, np.random.default_rng(8), b)
    for tau in (1.0, 0.62, 0.0):
        plain = aspace.search_batch(Q, gl, tau)
        got = aspace.search_batch_subset(Q, gl, tau, full)
        for i in range(b):
            same_as_single(got[i], plain[i])
        st, lists, lq, stt, ln = raw_batch(asp, aspace, gl, Q, tau, full, topk)
        assert st == 0 and not stt.any() and (ln == topk).all() and lists == got
        idx = np.empty((b, topk), dtype=np.int64)
        sc = np.empty((b, topk))
        ln2, lq2, st2 = np.zeros(b, dtype=np.int64), np.zeros(b), np.zeros(b, dtype=np.int32)
        assert asp._L.as_search_batch(aspace._h, gl._h, Q.ctypes.data, b, d, float(tau), idx.ctypes.data, sc.ctypes.data, ln2.ctypes.data,
                                      lq2.ctypes.data, st2.ctypes.data) == 0
        assert np.array_equal(lq, lq2)   # the same call underneath: bit-equal


# ---------------------------------------------------------------- 7. ties
def with_copies(q, Q_other):
    """three copies of q with two other queries between them"""
    return np.ascontiguousarray(np.stack([q, Q_other[0], q, Q_other[1], q]))


def test_exact_ties_come_back_in_index_order():
    import pyarrowspace_amd as asp
    n, d = 1000, 40
    X = clustered(n, d, nclust=8, seed=6)
    X[500] = X[10]
    X[900] = X[10]
    gp = {"eps": calibrate_eps(X, 8), "k": 8, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    other, _ = draw_queries(aspace, gl, X, np.random.default_rng(34), 2)
    Q = with_copies(np.ascontiguousarray(X[10] * 1.01), other)
    rest = [i for i in range(999, -1, -7) if i not in (10, 500, 900)]
    got = aspace.search_batch_subset(Q, gl, 1.0, [900, 500] + rest + [10])
    for c in (0, 2, 4):
        assert [i for i, _ in got[c][:3]] == [10, 500, 900]
        assert got[c][0][1] == got[c][1][1] == got[c][2][1]
        assert got[c][3][1] < got[c][2][1]
    assert got[0] == got[2] == got[4]
    sc = aspace.score_items_batch(Q, gl, 1.0, [900, 10, 500])
    for c in (0, 2, 4):
        assert sc[c, 0] == sc[c, 1] == sc[c, 2] == got[c][0][1]


def test_a_run_of_equal_scores_across_the_threshold_of_the_radix_select():
    """The 200 half-scaled copies of row 20 (test_gpu_subset.py): the threshold of the selection falls inside the run."""
    import pyarrowspace_amd as asp
    n, d = 4000, 32
    X = clustered(n, d, nclust=16, seed=22)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}   # (before the copies: their distances are 0)
    X[1000:1200] = 0.5 * X[20]
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    q = np.ascontiguousarray(X[20] * 1.01)
    assert aspace.query_lambda(q, gl) != 0.0
    other, _ = draw_queries(aspace, gl, X, np.random.default_rng(35), 2)
    Q = with_copies(q, other)
    got = aspace.search_batch_subset(Q, gl, 1.0, np.arange(n))
    for c in (0, 2, 4):
        assert [i for i, _ in got[c]] == [20, 1000, 1001, 1002, 1003]
        assert len({s for _, s in got[c]}) == 1
    assert got[0] == got[2] == got[4]
    got = aspace.search_batch_subset(Q, gl, 1.0, np.arange(n - 1, 499, -1))
    for c in (0, 2, 4):
        assert [i for i, _ in got[c]] == [1000, 1001, 1002, 1003, 1004]
        assert len({s for _, s in got[c]}) == 1
    assert got[0] == got[2] == got[4]


@pytest.mark.parametrize("first,last,topk", [(3800, 4400, 300), (3900, 5000, 1024)])
def test_a_run_of_equal_scores_that_reaches_the_position_digits(first, last, topk):
    """test_gpu_subset.py's wide runs (600 ties at ids 3800 .. 4399 with topk = 300, 1100 at 3900 .. 4999 with topk = 1024): the
    threshold lies inside the run and the run crosses position 4096, so digit 6 of the key decides -- in every row of the batched
    selection."""
    from test_gpu_subset import wide_tie_run
    aspace, gl, X, q, winners = wide_tie_run(first, last, topk)
    n = X.shape[0]
    other = np.ascontiguousarray(X[77] * 1.01)
    Q = np.stack([q, other, q])
    assert aspace.query_lambda(other, gl) != 0.0
    got = aspace.search_batch_subset(Q, gl, 1.0, np.arange(n))
    for c in (0, 2):
        assert [i for i, _ in got[c]] == winners
        assert len({np.float64(v).view(np.uint64).item() for _, v in got[c]}) == 1
    assert got[0] == got[2] and got[1] != got[0]
    S = aspace.score_items_batch(Q, gl, 1.0, np.arange(n))
    order = np.lexsort((np.arange(n), -(S[1] + 0.0)))[:topk]
    assert [i for i, _ in got[1]] == order.tolist()


# ---------------------------------------------------------------- 8. score_items_batch
@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
def test_score_items_batch(f32):
    import pyarrowspace_amd as asp
    n, d, k, topk, b = 2500, 200, 12, 20, 6
    X = clustered(n, d, nclust=24, seed=3)
    if f32:
        X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
    gp = {"eps": calibrate_eps(X, k), "k": k, "topk": topk, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    lam = aspace.lambdas()
    rng = np.random.default_rng(36)
    Q, lqs = draw_queries(aspace, gl, X, rng, b)
    sub_ids = rng.choice(n, 1500, replace=False)
    sub = aspace.subset(sub_ids)
    for tau in (1.0, 0.62, 0.0):
        hits = aspace.search_batch_subset(Q, gl, tau, sub)
        mixed = np.concatenate([rng.integers(0, n, 300), [0, n - 1, 0]])
        got = aspace.score_items_batch(Q, gl, tau, mixed)
        assert got.dtype == np.float64 and got.shape == (b, len(mixed))
        for i in range(b):
            np.testing.assert_allclose(got[i], np_scores(X, lam, lqs[i], Q[i], tau)[mixed], rtol=RTOL, atol=atol_for(d))
            np.testing.assert_allclose(got[i], aspace.score_items(Q[i], gl, tau, mixed), rtol=1e-12, atol=0.0)
            assert got[i, -3] == got[i, -1]   # a duplicate id: bit-equal
        # the scores search_batch_subset returned for the same (query, item) pairs: bit-equal, whatever the tile position.  Every
        # query's hits go into one id list, so each row holds its own query's hits among the others'
        flat = np.array([j for h in hits for j, _ in h], dtype=np.int64)
        again = aspace.score_items_batch(Q, gl, tau, flat)
        for i in range(b):
            assert again[i, i * topk:(i + 1) * topk].tolist() == [s for _, s in hits[i]]
    assert aspace.score_items_batch(Q, gl, 0.5, []).shape == (b, 0)
    assert aspace.score_items_batch(Q, gl, 0.5, np.zeros(n, dtype=bool)).shape == (b, 0)


# ---------------------------------------------------------------- 9. zero-norm row, topk edges, feature-lambda index
def test_zero_norm_row_scores_its_lambda_term():
    import pyarrowspace_amd as asp
    n, d, tau = 900, 24, 0.62
    X = clustered(n, d, nclust=8, seed=17)
    X[5] = 0.0
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 12, "p": 2.0, "sigma": None, "metric": "l2"}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    lam = aspace.lambdas()
    other, olq = draw_queries(aspace, gl, X, np.random.default_rng(37), 3)
    q = np.ascontiguousarray(X[40] * 1.01)
    lq = aspace.query_lambda(q, gl)
    assert lq != 0.0
    Q = np.ascontiguousarray(np.vstack([q[None], other]))
    lqs = np.concatenate([[lq], olq])
    sc = [np_scores(X, lam, l, v, tau) for v, l in zip(Q, lqs)]
    order = np.argsort(-sc[0])
    ids = np.concatenate([order[:4], order[-4:], [5]])   # the zero row between rows of positive and of negative cosine
    got = check_batch(aspace, gl, Q, tau, ids, ids, sc, 12, d)
    rows = aspace.score_items_batch(Q, gl, tau, [5])
    for i in range(4):
        at = [j for j, _ in got[i]].index(5)
        assert got[i][at][1] == pytest.approx((1.0 - tau) / (1.0 + abs(lqs[i] - lam[5])), rel=1e-15)
        assert rows[i, 0] == got[i][at][1]


@pytest.mark.parametrize("topk", [1024, 1])
def test_topk_edges(topk):
    import pyarrowspace_amd as asp
    n, d = 5000, 32
    X = clustered(n, d, nclust=16, seed=15)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": topk, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    lam = aspace.lambdas()
    rng = np.random.default_rng(16)
    Q, lqs = draw_queries(aspace, gl, X, rng, 4)
    for m in (3000, 700):
        ids = rng.choice(n, m, replace=False)
        for tau in (1.0, 0.62):
            sc = [np_scores(X, lam, lq, q, tau) for q, lq in zip(Q, lqs)]
            got = check_batch(aspace, gl, Q, tau, ids, ids, sc, topk, d)
            assert all(len(h) == min(topk, m) for h in got)


def test_feature_lambda_index():
    import pyarrowspace_amd as asp
    n, d = 800, 24
    X = clustered(n, d, nclust=8, seed=18)
    gp = {"eps": calibrate_feature_eps(X, 6), "k": 6, "topk": 8, "p": 2.0, "sigma": None, "metric": "cosine", "kernel": "rational",
          "lambda_mode": "feature"}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    assert gl.lambda_mode == "feature"
    lam = aspace.lambdas()
    rng = np.random.default_rng(19)
    ids = rng.choice(n, 200, replace=False)
    Q, lqs = draw_queries(aspace, gl, X, rng, 4)
    for tau in (1.0, 0.62, 0.0):
        sc = [np_scores(X, lam, lq, q, tau) for q, lq in zip(Q, lqs)]
        check_batch(aspace, gl, Q, tau, ids, ids, sc, 8, d)
        full = aspace.search_batch_subset(Q, gl, tau, np.arange(n))
        for i in range(4):
            same_as_single(full[i], aspace.search(Q[i], gl, tau))


# ---------------------------------------------------------------- 10. errors and edges
def test_errors_and_edges():
    import pyarrowspace_amd as asp
    n, d = 800, 32
    X = clustered(n, d, nclust=8, seed=4)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    other, gl2 = asp.ArrowSpaceBuilder.build(gp, X[:400].copy())
    good, _ = draw_queries(aspace, gl, X, np.random.default_rng(38), 3)
    far = np.full(d, 50.0)   # no item within eps: lambda_q == 0
    Q = np.ascontiguousarray(np.vstack([good[:2], far[None], good[2:]]))
    sub = aspace.subset([1, 2, 3, 700, 40])
    empty = aspace.subset([])
    for s in (sub, empty, [], [4, 5], np.arange(n)):
        with pytest.raises(asp.PanicException):
            aspace.search_batch_subset(Q, gl, 0.62, s)
    for ids in ([1, 2], []):
        with pytest.raises(asp.PanicException):
            aspace.score_items_batch(Q, gl, 0.62, ids)
    # through the C ABI: that query's status and length, the others' lists
    st, lists, lq, stt, ln = raw_batch(asp, aspace, gl, Q, 0.62, sub, 5)
    assert st == 0 and stt.tolist() == [0, 0, asp._lib.AS_EZEROLAMBDA, 0] and ln.tolist() == [5, 5, 0, 5] and lq[2] == 0.0
    for i in (0, 1, 3):
        same_as_single(lists[i], aspace.search_subset(np.ascontiguousarray(Q[i]), gl, 0.62, sub))
    st, lists, lq, stt, ln = raw_batch(asp, aspace, gl, Q, 0.62, empty, 0)
    assert st == 0 and stt.tolist() == [0, 0, asp._lib.AS_EZEROLAMBDA, 0] and ln.tolist() == [0, 0, 0, 0]
    out = np.full((4, 2), -5.0)
    lq4, st4 = np.zeros(4), np.zeros(4, dtype=np.int32)
    ids2 = np.array([3, 1], dtype=np.int64)
    assert asp._L.as_score_items_batch(aspace._h, gl._h, Q.ctypes.data, 4, d, 0.62, ids2.ctypes.data, 2, out.ctypes.data, lq4.ctypes.data,
                                       st4.ctypes.data) == 0
    assert st4.tolist() == [0, 0, asp._lib.AS_EZEROLAMBDA, 0] and out[2].tolist() == [-5.0, -5.0]   # left unwritten
    for i in (0, 1, 3):
        np.testing.assert_allclose(out[i], aspace.score_items(np.ascontiguousarray(Q[i]), gl, 0.62, ids2), rtol=1e-12, atol=0.0)
    # the single forms' errors
    with pytest.raises(ValueError, match="query length"):
        aspace.search_batch_subset(np.ascontiguousarray(good[:, :10]), gl, 0.62, sub)
    with pytest.raises(ValueError, match="query length"):
        aspace.score_items_batch(np.ascontiguousarray(good[:, :10]), gl, 0.62, [1, 2])
    with pytest.raises(ValueError, match="tau"):
        aspace.search_batch_subset(good, gl, float("nan"), sub)
    with pytest.raises(ValueError, match="tau"):
        aspace.score_items_batch(good, gl, float("inf"), [1, 2])
    with pytest.raises(ValueError, match="another space"):
        other.search_batch_subset(np.ascontiguousarray(good), gl2, 0.62, sub)
    for bad in ([0, n], [-1, 3]):
        with pytest.raises(ValueError):
            aspace.search_batch_subset(good, gl, 0.62, bad)
        with pytest.raises(ValueError, match="id"):
            aspace.score_items_batch(good, gl, 0.62, bad)
    with pytest.raises(TypeError):
        aspace.score_items_batch(good, gl, 0.62, [1.5])
    with pytest.raises(TypeError):
        aspace.search_batch_subset(good[0], gl, 0.62, sub)
    with pytest.raises(TypeError):
        aspace.score_items_batch(good[0], gl, 0.62, [1, 2])
    with pytest.raises(TypeError):
        aspace.search_batch_subset(good, None, 0.62, sub)
    # B == 0, the empty subset
    none = np.empty((0, d))
    assert aspace.search_batch_subset(none, gl, 0.62, sub) == []
    assert aspace.score_items_batch(none, gl, 0.62, [1, 2, 2]).shape == (0, 3)
    assert aspace.search_batch_subset(good, gl, 0.62, empty) == [[], [], []]
    assert aspace.search_batch_subset(good, gl, 0.62, []) == [[], [], []]
    assert aspace.search_batch_subset(good, gl, 0.62, np.zeros(n, dtype=bool)) == [[], [], []]
    assert [h[0][0] for h in aspace.search_batch_subset(np.ascontiguousarray(X[[3, 700]] * 1.01), gl, 1.0, sub)] == [3, 700]


# ---------------------------------------------------------------- 11. concurrency
def test_batched_and_single_calls_on_one_handle_from_several_threads(tiles):
    aspace, gl, Q, _, _, tau, _ = tiles
    rng = np.random.default_rng(39)
    ids = rng.choice(4000, 1500, replace=False)
    sub = aspace.subset(ids)
    Qb = np.ascontiguousarray(Q[:20])
    batched = aspace.search_batch_subset(Qb, gl, tau, sub)
    singles = [aspace.search_subset(q, gl, tau, sub) for q in Qb]
    plain = aspace.search_batch(Qb, gl, tau)
    for i in range(20):
        same_as_single(batched[i], singles[i])
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
        assert aspace.search_batch_subset(Qb, gl, tau, sub) == batched

    def f_single():
        assert [aspace.search_subset(q, gl, tau, sub) for q in Qb] == singles

    def f_plain():
        assert aspace.search_batch(Qb, gl, tau) == plain

    th = [run(f_batched), run(f_batched), run(f_single), run(f_plain)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]
