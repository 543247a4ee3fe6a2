"""GPU: per-query candidate lists -- ArrowSpace.search_batch_lists / score_lists_batch.  List i of the search form is what
`search_subset(items[i], gl, tau, lists[i])` returns, array i of the score form what `score_items(items[i], gl, tau, lists[i])`
returns: each is checked against the oracle's (or numpy's fp64) score of every item restricted to the list, at the project's
RTOL / atol_for(d), and against the single form at 1e-12 relative.  The bits of a score depend on its query, its row, tau and
lambda_q only: compared with `==` across positions, calls, chunk budgets and the two forms."""
import threading

import numpy as np
import pytest

from conftest import assert_hits_match, calibrate_eps, calibrate_feature_eps, clustered
from test_gpu_subset import RTOL, atol_for, expected, np_scores, same_as_single
from test_gpu_subset_batch import draw_queries

pytestmark = pytest.mark.gpu

R = 64   # entries per segment of the ragged score kernel (LISTS_R)


def check_lists(aspace, gl, Q, tau, lists, all_scores, topk, d, single=False):
    """Both forms over `lists` (one per query) against all_scores[i], the reference score of every item for query i."""
    got = aspace.search_batch_lists(Q, gl, tau, lists)
    rows = aspace.score_lists_batch(Q, gl, tau, lists)
    assert len(got) == len(rows) == len(Q)
    for i, (hits, row) in enumerate(zip(got, rows)):
        ids = np.asarray(lists[i], dtype=np.int64)
        uniq = set(np.unique(ids).tolist())
        assert len(hits) == min(topk, len(uniq))
        assert all(j in uniq for j, _ in hits)
        assert_hits_match(hits, expected(all_scores[i], ids, topk), all_scores[i], rtol=RTOL, atol=atol_for(d))
        assert row.dtype == np.float64 and row.shape == ids.shape
        np.testing.assert_allclose(row, all_scores[i][ids], rtol=RTOL, atol=atol_for(d))
        at = {int(j): float(s) for j, s in zip(ids, row)}
        assert all(at[j] == s for j, s in hits)   # the two forms: the same bits
        if single:
            q = np.ascontiguousarray(Q[i])
            same_as_single(hits, aspace.search_subset(q, gl, tau, ids))
            np.testing.assert_allclose(row, aspace.score_items(q, gl, tau, ids), rtol=1e-12, atol=0.0)
    return got, rows


def raw_scores(asp, aspace, gl, Q, tau, ids, offs, fill=np.nan):
    b = Q.shape[0]
    ids, offs = np.ascontiguousarray(ids, dtype=np.int64), np.ascontiguousarray(offs, dtype=np.int64)
    out = np.full(max(len(ids), 1), fill)
    lq = np.full(max(b, 1), -1.0)
    stt = np.full(max(b, 1), -7, dtype=np.int32)
    st = asp._L.as_score_lists_batch(aspace._h, gl._h, Q.ctypes.data, b, Q.shape[1], float(tau), ids.ctypes.data, offs.ctypes.data,
                                     out.ctypes.data, lq.ctypes.data, stt.ctypes.data)
    return st, out, lq, stt


def raw_search(asp, aspace, gl, Q, tau, ids, offs, kk):
    b = Q.shape[0]
    ids, offs = np.ascontiguousarray(ids, dtype=np.int64), np.ascontiguousarray(offs, dtype=np.int64)
    idx = np.full((b, kk), -1, dtype=np.int64)
    sc = np.full((b, kk), np.nan)
    ln = np.full(b, -1, dtype=np.int64)
    lq = np.full(b, -1.0)
    stt = np.full(b, -7, dtype=np.int32)
    st = asp._L.as_search_lists_batch(aspace._h, gl._h, Q.ctypes.data, b, Q.shape[1], float(tau), ids.ctypes.data, offs.ctypes.data,
                                      idx.ctypes.data, sc.ctypes.data, ln.ctypes.data, lq.ctypes.data, stt.ctypes.data)
    lists = [list(zip(idx[i, :max(ln[i], 0)].tolist(), sc[i, :max(ln[i], 0)].tolist())) for i in range(b)]
    return st, lists, lq, stt, ln, sc


# ---------------------------------------------------------------- 1. the oracle and the single form
@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
@pytest.mark.parametrize("n,d,k,topk,metric,kernel", [(1200, 48, 10, 10, "l2", "gaussian"), (3000, 96, 25, 10, "cosine", "rational"),
                                                       (1500, 51, 8, 6, "l2", "gaussian")])
def test_lists_match_oracle_and_single(oracle_lib, n, d, k, topk, metric, kernel, f32):
    import pyarrowspace_amd as asp
    X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
    if f32:
        X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
    gp = {"eps": calibrate_eps(X, k, metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    ref = oracle_lib.OracleIndex(X, gp)
    rng = np.random.default_rng(7)
    Q, _ = draw_queries(aspace, gl, X, rng, 6)
    lqs = [ref.search(q, 1.0)[1] for q in Q]
    lists = [np.empty(0, dtype=np.int64), rng.integers(0, n, 1), rng.choice(n, 7, replace=False), rng.choice(n, 300, replace=False),
             rng.permutation(n), rng.permutation(np.repeat(np.arange(n), 2))]
    every = [np.arange(n)] * 6
    for tau in (1.0, 0.62, 0.0):
        sc = [ref.scores(q, tau, lq) for q, lq in zip(Q, lqs)]
        check_lists(aspace, gl, Q, tau, lists, sc, topk, d, single=True)
        check_lists(aspace, gl, Q, tau, lists[::-1], sc, topk, d)   # every list with another query
        # every item listed: search_batch's lists outside ties
        plain = aspace.search_batch(Q, gl, tau)
        for hits, want in zip(aspace.search_batch_lists(Q, gl, tau, every), plain):
            same_as_single(hits, want)


# ---------------------------------------------------------------- 2. segment and selection edges
EDGE_M = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1024, 1025, 2047, 2049, 4000]
assert {R - 1, R + 1, 2 * R - 1, 2 * R + 1} <= set(EDGE_M)


@pytest.fixture(scope="module")
def edges():
    """n = 4000, d = 64, 130 queries and numpy's fp64 score of every item for each, computed once."""
    import pyarrowspace_amd as asp
    n, d, tau = 4000, 64, 0.62
    X = clustered(n, d, nclust=32, seed=20)
    gp = {"eps": calibrate_eps(X, 10), "k": 10, "topk": 10, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(41)
    Q, lqs = draw_queries(aspace, gl, X, rng, 130)
    lam = aspace.lambdas()
    sc = [np_scores(X, lam, lq, q, tau) for q, lq in zip(Q, lqs)]
    return aspace, gl, Q, sc, tau, d, n


@pytest.mark.parametrize("order", ["ascending lengths", "descending lengths"])
def test_segment_and_selection_edges(edges, order):
    aspace, gl, Q, sc, tau, d, n = edges
    rng = np.random.default_rng(42)
    lists = [rng.choice(n, m, replace=False) for m in EDGE_M]
    if order == "descending lengths":
        lists = lists[::-1]
    b = len(lists)
    check_lists(aspace, gl, np.ascontiguousarray(Q[:b]), tau, lists, sc[:b], 10, d)


def test_many_lists_of_one_odd_length(edges):
    aspace, gl, Q, sc, tau, d, n = edges
    rng = np.random.default_rng(43)
    lists = [rng.choice(n, 129, replace=False) for _ in range(130)]
    check_lists(aspace, gl, Q, tau, lists, sc, 10, d)
    as_array = np.stack(lists)
    rows = aspace.score_lists_batch(Q, gl, tau, as_array)   # a 2-D array in, a 2-D array out
    assert isinstance(rows, np.ndarray) and rows.shape == (130, 129)
    assert np.array_equal(rows, np.stack(aspace.score_lists_batch(Q, gl, tau, lists)))
    assert aspace.search_batch_lists(Q, gl, tau, as_array) == aspace.search_batch_lists(Q, gl, tau, lists)


# ---------------------------------------------------------------- 3. independence, bitwise
def test_scores_do_not_depend_on_the_call(edges):
    """40 lists of 4000 entries: 1.28 MB of scores, two chunks under a budget of 1 MiB."""
    import pyarrowspace_amd as asp
    aspace, gl, Q, _, tau, d, n = edges
    rng = np.random.default_rng(44)
    lists = [rng.permutation(n) for _ in range(40)]
    Q40 = np.ascontiguousarray(Q[:40])
    whole = aspace.score_lists_batch(Q40, gl, tau, lists)
    hits = aspace.search_batch_lists(Q40, gl, tau, lists)
    in33 = aspace.score_lists_batch(np.ascontiguousarray(Q[:33]), gl, tau, lists[:33])
    try:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 1) == 0
        before = aspace.lists_counters()
        chunked = aspace.score_lists_batch(Q40, gl, tau, lists)
        after = aspace.lists_counters()
        chunked_hits = aspace.search_batch_lists(Q40, gl, tau, lists)
    finally:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 256) == 0
    assert after["calls"] - before["calls"] == 1 and after["lambda_steps"] - before["lambda_steps"] == 1
    assert after["score_launches"] - before["score_launches"] >= 2
    assert after["pairs"] - before["pairs"] == 40 * n
    assert chunked_hits == hits
    for i in (0, 17, 32, 39):
        alone = aspace.score_lists_batch(np.ascontiguousarray(Q[i:i + 1]), gl, tau, [lists[i]])[0]
        # the same list in another order, after another list: another position, another segment
        moved = aspace.score_lists_batch(np.ascontiguousarray(Q[[3, i]]), gl, tau, [lists[5][:77], lists[i][::-1]])[1][::-1]
        for other in [alone, moved, chunked[i]] + ([in33[i]] if i < 33 else []):
            assert np.array_equal(whole[i].view(np.int64), other.view(np.int64))
        at = dict(zip(lists[i].tolist(), whole[i].tolist()))
        assert len(hits[i]) == 10 and all(at[j] == s for j, s in hits[i])


# ---------------------------------------------------------------- 4. ties and order
def test_exact_ties_come_back_in_index_order():
    import pyarrowspace_amd as asp
    n, d = 1000, 40
    X = clustered(n, d, nclust=8, seed=6)
    X[500] = X[10]
    X[900] = X[10]
    gp = {"eps": calibrate_eps(X, 8), "k": 8, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    other, _ = draw_queries(aspace, gl, X, np.random.default_rng(34), 2)
    q = np.ascontiguousarray(X[10] * 1.01)
    Q = np.ascontiguousarray(np.stack([q, other[0], q, other[1]]))
    down = np.arange(n - 1, -1, -1)                        # descending ids: 900 before 500 before 10
    twice = np.repeat(np.arange(0, n, 2), 2)               # every even id two times in a row
    lists = [down, down[:400], twice, twice]
    got = aspace.search_batch_lists(Q, gl, 1.0, lists)
    for c in (0, 2):
        assert [i for i, _ in got[c][:3]] == [10, 500, 900]
        assert got[c][0][1] == got[c][1][1] == got[c][2][1]
        assert got[c][3][1] < got[c][2][1]
    assert got[0][:3] == got[2][:3]
    for hits, ids in zip(got, lists):   # duplicates appear once
        assert len(hits) == 5 and len({i for i, _ in hits}) == 5 and all(i in set(ids.tolist()) for i, _ in hits)
    rows = aspace.score_lists_batch(Q, gl, 1.0, lists)
    assert rows[0][n - 1 - 10] == rows[0][n - 1 - 500] == rows[0][n - 1 - 900] == got[0][0][1]
    for c in (2, 3):   # ... and at every position of the score form, with the same bits
        assert rows[c].shape == twice.shape and np.array_equal(rows[c][0::2], rows[c][1::2])
    assert rows[2][10] == rows[2][500] == rows[2][900] == got[0][0][1]


# ---------------------------------------------------------------- 5. d edges
@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
@pytest.mark.parametrize("d", [1, 3, 31, 33, 100, 4100])
def test_feature_count_edges(d, f32):
    """d = 4100: the query does not fit the LDS staging and is read from global memory."""
    import pyarrowspace_amd as asp
    n, b, tau = (300, 5, 0.62) if d > 4096 else (900, 9, 0.62)
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
    lists = [rng.choice(n, m, replace=False) for m in ([200, 1, 67, n, 130] + [50, 3, 64, 199])[:b]]
    check_lists(aspace, gl, Q, tau, lists, sc, 7, d, single=True)


# ---------------------------------------------------------------- 6. a zero-norm item, a feature-lambda index
def test_zero_norm_row_scores_its_lambda_term():
    import pyarrowspace_amd as asp
    n, d, tau = 900, 24, 0.62
    X = clustered(n, d, nclust=8, seed=17)
    X[5] = 0.0
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 12, "p": 2.0, "sigma": None, "metric": "l2"}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    lam = aspace.lambdas()
    Q, lqs = draw_queries(aspace, gl, X, np.random.default_rng(37), 4)
    sc = [np_scores(X, lam, l, v, tau) for v, l in zip(Q, lqs)]
    lists = []
    for s in sc:
        order = np.argsort(-s)
        lists.append(np.concatenate([order[:4], order[-4:], [5]]))   # the zero row between rows of positive and of negative cosine
    got, rows = check_lists(aspace, gl, Q, tau, lists, sc, 12, d)
    for i in range(4):
        at = [j for j, _ in got[i]].index(5)
        assert got[i][at][1] == pytest.approx((1.0 - tau) / (1.0 + abs(lqs[i] - lam[5])), rel=1e-15)
        assert rows[i][-1] == got[i][at][1]


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
    Q, lqs = draw_queries(aspace, gl, X, rng, 4)
    lists = [rng.choice(n, m, replace=False) for m in (200, 5, 65, n)]
    for tau in (1.0, 0.62, 0.0):
        sc = [np_scores(X, lam, lq, q, tau) for q, lq in zip(Q, lqs)]
        check_lists(aspace, gl, Q, tau, lists, sc, 8, d, single=True)


# ---------------------------------------------------------------- 7. a zero-lambda query in the middle of a batch
def test_a_zero_lambda_query_is_skipped_and_its_neighbours_served():
    import pyarrowspace_amd as asp
    n, d, tau = 800, 32, 0.62
    X = clustered(n, d, nclust=8, seed=4)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    good, _ = draw_queries(aspace, gl, X, np.random.default_rng(38), 3)
    far = np.full(d, 50.0)   # no item within eps: lambda_q == 0
    Q = np.ascontiguousarray(np.vstack([good[:2], far[None], good[2:]]))
    rng = np.random.default_rng(45)
    lists = [rng.choice(n, 70, replace=False), rng.choice(n, 3, replace=False), rng.choice(n, 130, replace=False), rng.choice(n, 9, replace=False)]
    ids, offs = asp._id_lists(lists, n)
    ZL = asp._lib.AS_EZEROLAMBDA
    st, out, lq, stt = raw_scores(asp, aspace, gl, Q, tau, ids, offs)
    assert st == 0 and stt.tolist() == [0, 0, ZL, 0] and lq[2] == 0.0 and (lq[[0, 1, 3]] != 0.0).all()
    assert np.isnan(out[offs[2]:offs[3]]).all()   # left unwritten
    for i in (0, 1, 3):
        np.testing.assert_allclose(out[offs[i]:offs[i + 1]], aspace.score_items(np.ascontiguousarray(Q[i]), gl, tau, lists[i]), rtol=1e-12, atol=0.0)
    st, hits, lq2, stt, ln, _ = raw_search(asp, aspace, gl, Q, tau, ids, offs, 5)
    assert st == 0 and stt.tolist() == [0, 0, ZL, 0] and ln.tolist() == [5, 3, 0, 5] and np.array_equal(lq, lq2)
    for i in (0, 1, 3):
        same_as_single(hits[i], aspace.search_subset(np.ascontiguousarray(Q[i]), gl, tau, lists[i]))
    st, _, _, stt = raw_scores(asp, aspace, gl, Q, tau, [], [0, 0, 0, 0, 0])   # empty lists still run the lambda_q step
    assert st == 0 and stt.tolist() == [0, 0, ZL, 0]
    for ls in (lists, [[], [], [], []]):
        with pytest.raises(asp.PanicException):
            aspace.search_batch_lists(Q, gl, tau, ls)
        with pytest.raises(asp.PanicException):
            aspace.score_lists_batch(Q, gl, tau, ls)


# ---------------------------------------------------------------- 8. errors and edges
def test_errors_and_edges():
    import pyarrowspace_amd as asp
    n, d = 800, 32
    X = clustered(n, d, nclust=8, seed=4)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    good, _ = draw_queries(aspace, gl, X, np.random.default_rng(38), 3)
    lists = [[1, 2, 3], [700, 40], []]
    assert [len(h) for h in aspace.search_batch_lists(good, gl, 0.62, lists)] == [3, 2, 0]
    before = aspace.lists_counters()
    for bad, name in (([[1, 2], [3, -1], [4]], "-1"), ([[1, 2], [3], [4, n]], str(n))):
        for f in (aspace.search_batch_lists, aspace.score_lists_batch):
            with pytest.raises(ValueError, match=f"id {name} of list"):
                f(good, gl, 0.62, bad)
    with pytest.raises(ValueError, match="query length"):
        aspace.search_batch_lists(np.ascontiguousarray(good[:, :10]), gl, 0.62, lists)
    with pytest.raises(ValueError, match="query length"):
        aspace.score_lists_batch(np.ascontiguousarray(good[:, :10]), gl, 0.62, lists)
    with pytest.raises(ValueError, match="tau"):
        aspace.search_batch_lists(good, gl, float("nan"), lists)
    with pytest.raises(ValueError, match="tau"):
        aspace.score_lists_batch(good, gl, float("nan"), lists)
    for f in (aspace.search_batch_lists, aspace.score_lists_batch):
        with pytest.raises(ValueError, match="id lists"):
            f(good, gl, 0.62, lists[:2])
        with pytest.raises(TypeError):
            f(good, gl, 0.62, [[1.5], [1], [2]])
        with pytest.raises(TypeError):
            f(good[0], gl, 0.62, lists)
        with pytest.raises(TypeError):
            f(good, None, 0.62, lists)
    EINVAL = asp._lib.AS_EINVAL
    ids = np.array([1, 2, 3, 4], dtype=np.int64)
    for offs in ([0, 3, 2, 4], [1, 2, 3, 4]):   # decreasing; not starting at 0
        st, out, _, _ = raw_scores(asp, aspace, gl, good, 0.62, ids, offs, fill=-5.0)
        assert st == EINVAL and "offsets" in asp._lib.last_error() and (out == -5.0).all()
        assert raw_search(asp, aspace, gl, good, 0.62, ids, offs, 5)[0] == EINVAL
    assert aspace.lists_counters() == before   # every one of them was refused before the lambda_q step
    # B == 0, empty lists
    none = np.empty((0, d))
    assert aspace.search_batch_lists(none, gl, 0.62, []) == []
    assert aspace.score_lists_batch(none, gl, 0.62, []) == []
    assert aspace.score_lists_batch(none, gl, 0.62, np.empty((0, 3), dtype=np.int64)).shape == (0, 3)
    assert aspace.lists_counters()["lambda_steps"] == before["lambda_steps"]
    assert aspace.search_batch_lists(good, gl, 0.62, [[], [], []]) == [[], [], []]
    assert [r.shape for r in aspace.score_lists_batch(good, gl, 0.62, [[], [], []])] == [(0,)] * 3
    assert aspace.lists_counters()["lambda_steps"] == before["lambda_steps"] + 2
    masks = [np.zeros(n, dtype=bool) for _ in range(3)]
    masks[1][[3, 700]] = True
    assert [[i for i, _ in h] for h in aspace.search_batch_lists(np.ascontiguousarray(X[[1, 3, 5]] * 1.01), gl, 1.0, masks)] == [[], [3, 700], []]


# ---------------------------------------------------------------- 9. concurrency
def test_two_threads_on_one_space(edges):
    aspace, gl, Q, _, tau, _, n = edges
    rng = np.random.default_rng(46)
    Qb = np.ascontiguousarray(Q[:12])
    lists = [rng.choice(n, m, replace=False) for m in (5, 64, 700, 1500, 1, 130, 4000, 33, 0, 250, 1025, 90)]
    hits = aspace.search_batch_lists(Qb, gl, tau, lists)
    rows = aspace.score_lists_batch(Qb, gl, tau, lists)
    errors = []

    def body(search):
        try:
            for _ in range(8):
                if search:
                    assert aspace.search_batch_lists(Qb, gl, tau, lists) == hits
                else:
                    got = aspace.score_lists_batch(Qb, gl, tau, lists)
                    assert all(np.array_equal(g.view(np.int64), r.view(np.int64)) for g, r in zip(got, rows))
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=body, args=(True,)), threading.Thread(target=body, args=(False,))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]
