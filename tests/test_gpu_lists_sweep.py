"""GPU: tau sweeps over per-query candidate lists -- ArrowSpace.search_batch_lists_taus / score_lists_batch_taus.  Entry [i][j] of
either is what the single-tau form (`search_batch_lists` / `score_lists_batch`) returns for query i under taus[j]: checked against
the oracle's (or numpy's fp64) score of every item restricted to the list at the project's RTOL / atol_for(d), against the
single-tau forms at 1e-12 relative (with `==` for taus[0], where both run the same lambda_q step), and with `==` within one call,
across tau groups and across chunk budgets."""
import threading

import numpy as np
import pytest

from conftest import assert_hits_match, calibrate_eps, calibrate_feature_eps, clustered
from test_gpu_lists import EDGE_M, edges  # noqa: F401  (the fixture: n = 4000, d = 64, 130 queries)
from test_gpu_subset import RTOL, atol_for, expected, np_scores, same_as_single
from test_gpu_subset_batch import draw_queries

pytestmark = pytest.mark.gpu

TAUS = [1.0, 0.62, 0.0]
GROUP = 8   # taus per gather (TAU_GROUP)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def check_sweep(aspace, gl, Q, taus, lists, ref, topk, d):
    """Both sweep forms over `lists` (one per query) against ref(i, tau), the reference score of every item for query i."""
    got = aspace.search_batch_lists_taus(Q, gl, taus, lists)
    rows = aspace.score_lists_batch_taus(Q, gl, taus, lists)
    assert len(got) == len(rows) == len(Q)
    for i in range(len(Q)):
        ids = np.asarray(lists[i], dtype=np.int64)
        uniq = set(np.unique(ids).tolist())
        assert len(got[i]) == len(taus) and rows[i].dtype == np.float64 and rows[i].shape == (len(taus), len(ids))
        for j, tau in enumerate(taus):
            hits, row, want = got[i][j], rows[i][j], ref(i, tau)
            assert len(hits) == min(topk, len(uniq))
            assert all(t in uniq for t, _ in hits)
            assert_hits_match(hits, expected(want, ids, topk), want, rtol=RTOL, atol=atol_for(d))
            np.testing.assert_allclose(row, want[ids], rtol=RTOL, atol=atol_for(d))
            at = {int(t): float(s) for t, s in zip(ids, row)}
            assert all(at[t] == s for t, s in hits)   # the two forms: the same bits
    return got, rows


def check_against_single(aspace, gl, Q, taus, lists):
    """Every plane / list against the single-tau forms: 1e-12 relative, `==` for taus[0] (the same lambda_q step)."""
    got = aspace.search_batch_lists_taus(Q, gl, taus, lists)
    rows = aspace.score_lists_batch_taus(Q, gl, taus, lists)
    for j, tau in enumerate(taus):
        hits = aspace.search_batch_lists(Q, gl, tau, lists)
        single = aspace.score_lists_batch(Q, gl, tau, lists)
        for i in range(len(Q)):
            same_as_single(got[i][j], hits[i])
            np.testing.assert_allclose(rows[i][j], single[i], rtol=1e-12, atol=0.0)
            if j == 0:
                assert got[i][0] == hits[i]
                assert np.array_equal(bits(rows[i][0]), bits(single[i]))
    return got, rows


def raw_scores(asp, aspace, gl, Q, taus, ids, offs, fill=np.nan):
    b, taus = Q.shape[0], np.ascontiguousarray(taus, dtype=np.float64)
    ids, offs = np.ascontiguousarray(ids, dtype=np.int64), np.ascontiguousarray(offs, dtype=np.int64)
    out = np.full(max(len(ids) * len(taus), 1), fill)
    lq = np.full(max(b, 1), -1.0)
    stt = np.full(max(b, 1), -7, dtype=np.int32)
    st = asp._L.as_score_lists_batch_taus(aspace._h, gl._h, Q.ctypes.data, b, Q.shape[1], taus.ctypes.data, len(taus), ids.ctypes.data,
                                          offs.ctypes.data, out.ctypes.data, lq.ctypes.data, stt.ctypes.data)
    return st, out, lq, stt


def raw_search(asp, aspace, gl, Q, taus, ids, offs, kk):
    b, taus = Q.shape[0], np.ascontiguousarray(taus, dtype=np.float64)
    nt = len(taus)
    ids, offs = np.ascontiguousarray(ids, dtype=np.int64), np.ascontiguousarray(offs, dtype=np.int64)
    idx = np.full((b, nt, kk), -1, dtype=np.int64)
    sc = np.full((b, nt, kk), np.nan)
    ln = np.full((b, nt), -1, dtype=np.int64)
    lq = np.full(b, -1.0)
    stt = np.full(b, -7, dtype=np.int32)
    st = asp._L.as_search_lists_batch_taus(aspace._h, gl._h, Q.ctypes.data, b, Q.shape[1], taus.ctypes.data, nt, ids.ctypes.data,
                                           offs.ctypes.data, idx.ctypes.data, sc.ctypes.data, ln.ctypes.data, lq.ctypes.data, stt.ctypes.data)
    lists = [[list(zip(idx[i, j, :max(ln[i, j], 0)].tolist(), sc[i, j, :max(ln[i, j], 0)].tolist())) for j in range(nt)] for i in range(b)]
    return st, lists, lq, stt, ln


@pytest.fixture(scope="module")
def swept(edges):  # noqa: F811
    """The `edges` index with what a reference for other taus needs: the items, their lambdas and lambda_q of every query."""
    aspace, gl, Q, _, _, d, n = edges
    X = clustered(n, d, nclust=32, seed=20)   # (the fixture's items)
    lam = aspace.lambdas()
    lqs = np.array([aspace.query_lambda(np.ascontiguousarray(q), gl) for q in Q])
    cache = {}

    def ref(i, tau):
        if (i, tau) not in cache:
            cache[(i, tau)] = np_scores(X, lam, lqs[i], Q[i], tau)
        return cache[(i, tau)]

    return aspace, gl, Q, ref, d, n


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
@pytest.mark.parametrize("n,d,k,topk,metric,kernel", [(1200, 48, 10, 10, "l2", "gaussian"), (3000, 96, 25, 10, "cosine", "rational")])
def test_sweeps_match_the_oracle(oracle_lib, n, d, k, topk, metric, kernel, f32):
    import pyarrowspace_amd as asp
    X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
    if f32:
        X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
    gp = {"eps": calibrate_eps(X, k, metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    oracle = oracle_lib.OracleIndex(X, gp)
    rng = np.random.default_rng(7)
    Q, _ = draw_queries(aspace, gl, X, rng, 6)
    lqs = [oracle.search(q, 1.0)[1] for q in Q]
    lists = [np.empty(0, dtype=np.int64), rng.integers(0, n, 1), rng.choice(n, 7, replace=False), rng.choice(n, 300, replace=False),
             rng.permutation(n), rng.permutation(np.repeat(np.arange(n), 2))]
    sc = {(i, tau): oracle.scores(Q[i], tau, lqs[i]) for i in range(6) for tau in TAUS}
    check_sweep(aspace, gl, Q, TAUS, lists, lambda i, tau: sc[(i, tau)], topk, d)
    check_sweep(aspace, gl, Q, TAUS, lists[::-1], lambda i, tau: sc[(i, tau)], topk, d)   # every list with another query


# ---------------------------------------------------------------- 2. the single-tau forms
def test_sweeps_agree_with_the_single_tau_forms(swept):
    aspace, gl, Q, _, _, n = swept
    rng = np.random.default_rng(47)
    lens = (0, 1, 7, 63, 64, 65, 300, 1024, 1025, 4000)
    lists = [rng.choice(n, m, replace=False) for m in lens] + [rng.permutation(np.repeat(np.arange(0, n, 3), 2))]
    check_against_single(aspace, gl, np.ascontiguousarray(Q[:len(lists)]), [0.62, 1.0, 0.0, 0.3], lists)


# ---------------------------------------------------------------- 3. within one call, bitwise
def test_duplicates_repeated_taus_and_group_boundaries_bitwise(swept):
    aspace, gl, Q, _, _, n = swept
    rng = np.random.default_rng(48)
    twice = np.repeat(rng.choice(n, 700, replace=False), 2)   # every id two times in a row
    lists = [twice, rng.choice(n, 1500, replace=False), rng.choice(n, 70, replace=False), twice[::-1]]
    Q4 = np.ascontiguousarray(Q[:4])
    rows = aspace.score_lists_batch_taus(Q4, gl, TAUS, lists)
    hits = aspace.search_batch_lists_taus(Q4, gl, TAUS, lists)
    for i in range(4):
        for j in range(3):
            at = dict(zip(lists[i].tolist(), rows[i][j].tolist()))
            assert len(hits[i][j]) == 10 and all(at[t] == s for t, s in hits[i][j])   # the search form's scores: the score form's bits
    for c in (0, 3):   # an id listed twice: the same bits twice in every plane
        assert np.array_equal(bits(rows[c][:, 0::2]), bits(rows[c][:, 1::2]))
    # repeated taus: equal planes and lists
    rep = aspace.score_lists_batch_taus(Q4, gl, [0.62, 1.0, 0.62], lists)
    rep_hits = aspace.search_batch_lists_taus(Q4, gl, [0.62, 1.0, 0.62], lists)
    for i in range(4):
        assert np.array_equal(bits(rep[i][0]), bits(rep[i][2])) and rep_hits[i][0] == rep_hits[i][2]
        assert np.array_equal(bits(rep[i][0]), bits(rows[i][1])) and np.array_equal(bits(rep[i][1]), bits(rows[i][0]))
        assert rep_hits[i][0] == hits[i][1] and rep_hits[i][1] == hits[i][0]
    # a 9-tau sweep crosses a group boundary: its first three planes are the 3-tau sweep's (the lambda_q step is the same)
    nine = TAUS + [0.9, 0.8, 0.5, 0.25, 0.1, 0.7]
    rows9 = aspace.score_lists_batch_taus(Q4, gl, nine, lists)
    hits9 = aspace.search_batch_lists_taus(Q4, gl, nine, lists)
    for i in range(4):
        assert rows9[i].shape == (9, len(lists[i]))
        assert np.array_equal(bits(rows9[i][:3]), bits(rows[i])) and hits9[i][:3] == hits[i]
        at = dict(zip(lists[i].tolist(), rows9[i][8].tolist()))
        assert all(at[t] == s for t, s in hits9[i][8])   # the plane of the second group


def test_identical_rows_tie_in_index_order_for_every_tau():
    import pyarrowspace_amd as asp
    n, d = 1000, 40
    X = clustered(n, d, nclust=8, seed=6)
    X[500] = X[10]
    X[900] = X[10]
    gp = {"eps": calibrate_eps(X, 8), "k": 8, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    other, _ = draw_queries(aspace, gl, X, np.random.default_rng(34), 1)
    q = np.ascontiguousarray(X[10] * 1.01)
    Q = np.ascontiguousarray(np.stack([q, other[0], q]))
    down = np.arange(n - 1, -1, -1)   # descending ids: 900 before 500 before 10
    lists = [down, down[:400], np.array([900, 3, 500, 10, 77])]
    taus = [1.0, 0.62, 0.0, 1.0, 2.0]
    got = aspace.search_batch_lists_taus(Q, gl, taus, lists)
    rows = aspace.score_lists_batch_taus(Q, gl, taus, lists)
    for j in range(len(taus)):   # every tau: the order by (score descending, index ascending) of the score form's own bits
        for c in range(3):
            full = np.full(n, -np.inf)
            full[lists[c]] = rows[c][j]
            assert got[c][j] == expected(full, lists[c], 5)
    for j in (0, 3):   # tau = 1: the three identical rows tie bit for bit at the top
        for c in (0, 2):
            assert [i for i, _ in got[c][j][:3]] == [10, 500, 900]
            assert got[c][j][0][1] == got[c][j][1][1] == got[c][j][2][1] > got[c][j][3][1]
        assert rows[0][j][n - 1 - 10] == rows[0][j][n - 1 - 500] == rows[0][j][n - 1 - 900] == got[0][j][0][1]
        assert rows[2][j][0] == rows[2][j][2] == rows[2][j][3] == got[0][j][0][1]


# ---------------------------------------------------------------- 4. edges
@pytest.mark.parametrize("order", ["ascending lengths", "descending lengths"])
def test_segment_and_selection_edges(swept, order):
    aspace, gl, Q, ref, d, n = swept
    rng = np.random.default_rng(42)
    lists = [rng.choice(n, m, replace=False) for m in EDGE_M]
    if order == "descending lengths":
        lists = lists[::-1]
    check_sweep(aspace, gl, np.ascontiguousarray(Q[:len(lists)]), TAUS, lists, ref, 10, d)


@pytest.mark.parametrize("T", [1, 2, 8, 9, 16, 17])
def test_tau_counts_around_the_group_size(swept, T):
    aspace, gl, Q, ref, d, n = swept
    assert {GROUP, GROUP + 1, 2 * GROUP, 2 * GROUP + 1} <= {1, 2, 8, 9, 16, 17}
    rng = np.random.default_rng(49)
    lists = [rng.choice(n, 129, replace=False), rng.choice(n, 1025, replace=False)]
    taus = [round(1.0 - j / 17.0, 6) for j in range(T)]   # distinct
    check_sweep(aspace, gl, np.ascontiguousarray(Q[:2]), taus, lists, ref, 10, d)


@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
@pytest.mark.parametrize("d", [1, 3, 31, 33, 100, 4100])
def test_feature_count_edges(d, f32):
    """d = 4100 (n = 256): dp > 4096, the query does not fit the LDS staging and is read from global memory."""
    import pyarrowspace_amd as asp
    n, b = (256, 4) if d > 4096 else (900, 6)
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
    lists = [rng.choice(n, m, replace=False) for m in [200, 1, 67, n, 130, 64][:b]]
    check_sweep(aspace, gl, Q, TAUS, lists, lambda i, tau: np_scores(X, lam, lqs[i], Q[i], tau), 7, d)
    check_against_single(aspace, gl, Q, TAUS, lists)


def test_more_lists_than_one_block_round(swept):
    aspace, gl, Q, ref, d, n = swept
    rng = np.random.default_rng(43)
    lists = [rng.choice(n, 129, replace=False) for _ in range(130)]
    got, rows = check_sweep(aspace, gl, Q, TAUS, lists, ref, 10, d)
    as_array = np.stack(lists)
    cube = aspace.score_lists_batch_taus(Q, gl, TAUS, as_array)   # a 2-D array in, a 3-D array out
    assert isinstance(cube, np.ndarray) and cube.shape == (130, 3, 129)
    assert np.array_equal(bits(cube), bits(np.stack(rows)))
    assert aspace.search_batch_lists_taus(Q, gl, TAUS, as_array) == got


# ---------------------------------------------------------------- 5. the budget, 6. the counters
def test_results_do_not_depend_on_the_budget(swept):
    """40 lists of 4000 entries, nine taus: under 1 MiB (131072 scores) a chunk holds 4 lists at 8 taus a gather, and the ninth
    tau is a gather of its own: Tg = 8 < T in ten chunks.  Long lists with repeated ids (the score form keeps them): 40000
    entries leave Tg = 3 of T = 6, 140000 entries exceed the budget and run alone at Tg = 1, a list of 5 takes all six."""
    import pyarrowspace_amd as asp
    aspace, gl, Q, _, _, n = swept
    rng = np.random.default_rng(44)
    lists = [rng.permutation(n) for _ in range(40)]
    Q40 = np.ascontiguousarray(Q[:40])
    nine = TAUS + [0.9, 0.8, 0.5, 0.25, 0.1, 0.7]
    six = nine[:6]
    long_lists = [np.tile(lists[0], 10), np.tile(lists[1], 35), lists[2][:5]]
    Q3 = np.ascontiguousarray(Q[:3])
    whole = aspace.score_lists_batch_taus(Q40, gl, nine, lists)
    hits = aspace.search_batch_lists_taus(Q40, gl, nine, lists)
    c0 = aspace.lists_sweep_counters()
    long_whole = aspace.score_lists_batch_taus(Q3, gl, six, long_lists)
    c1 = aspace.lists_sweep_counters()
    try:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 1) == 0
        before = aspace.lists_sweep_counters()
        chunked = aspace.score_lists_batch_taus(Q40, gl, nine, lists)
        after = aspace.lists_sweep_counters()
        chunked_hits = aspace.search_batch_lists_taus(Q40, gl, nine, lists)
        c2 = aspace.lists_sweep_counters()
        long_chunked = aspace.score_lists_batch_taus(Q3, gl, six, long_lists)
        c3 = aspace.lists_sweep_counters()
    finally:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 256) == 0
    for i in range(40):
        assert np.array_equal(bits(whole[i]), bits(chunked[i]))
    assert chunked_hits == hits
    for i in range(3):
        assert np.array_equal(bits(long_whole[i]), bits(long_chunked[i]))
        head = min(n, len(long_lists[i]))   # list i of the 40 starts with the same ids: the same (query, tau, item)
        assert np.array_equal(bits(long_whole[i][:, :head]), bits(whole[i][:6, :head]))
    delta = {k: after[k] - before[k] for k in after}
    assert delta == {"calls": 1, "score_launches": 20, "pairs": 40 * n * 2, "scores": 40 * n * 9, "lambda_steps": 1}
    total = sum(len(l) for l in long_lists)
    assert {k: c1[k] - c0[k] for k in c1} == {"calls": 1, "score_launches": 1, "pairs": total, "scores": total * 6, "lambda_steps": 1}
    assert {k: c3[k] - c2[k] for k in c3} == {"calls": 1, "score_launches": 2 + 6 + 1, "pairs": 40000 * 2 + 140000 * 6 + 5,
                                              "scores": total * 6, "lambda_steps": 1}


def test_counters(swept):
    aspace, gl, Q, _, _, n = swept
    rng = np.random.default_rng(50)
    lens = (5, 0, 700, 64)
    lists = [rng.choice(n, m, replace=False) for m in lens]
    lists[2] = np.concatenate([lists[2], lists[2][:100]])   # 100 repeated ids: the search form scores 700 distinct ones
    Q4 = np.ascontiguousarray(Q[:4])
    single = aspace.lists_counters()
    before = aspace.lists_sweep_counters()
    aspace.score_lists_batch_taus(Q4, gl, [1.0, 0.62, 1.0, 0.0], lists)   # three distinct taus, one group
    mid = aspace.lists_sweep_counters()
    aspace.search_batch_lists_taus(Q4, gl, [round(0.05 * j, 2) for j in range(11)], lists)   # eleven: two groups
    after = aspace.lists_sweep_counters()
    assert {k: mid[k] - before[k] for k in mid} == {"calls": 1, "score_launches": 1, "pairs": 869, "scores": 869 * 3, "lambda_steps": 1}
    assert {k: after[k] - mid[k] for k in mid} == {"calls": 1, "score_launches": 2, "pairs": 769 * 2, "scores": 769 * 11, "lambda_steps": 1}
    assert aspace.lists_counters() == single   # the single-tau forms' counters do not see the sweeps


# ---------------------------------------------------------------- 7. errors and edges
def test_errors_and_edges():
    import pyarrowspace_amd as asp
    n, d = 800, 32
    X = clustered(n, d, nclust=8, seed=4)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    good, _ = draw_queries(aspace, gl, X, np.random.default_rng(38), 3)
    lists = [[1, 2, 3], [700, 40], []]
    forms = (aspace.search_batch_lists_taus, aspace.score_lists_batch_taus)
    assert [[len(h) for h in per] for per in aspace.search_batch_lists_taus(good, gl, TAUS, lists)] == [[3] * 3, [2] * 3, [0] * 3]
    before, single = aspace.lists_sweep_counters(), aspace.lists_counters()
    for f in forms:
        for bad_tau in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="tau"):
                f(good, gl, [1.0, bad_tau, 0.5], lists)
        for bad, name in (([[1, 2], [3, -1], [4]], "-1"), ([[1, 2], [3], [4, n]], str(n))):
            with pytest.raises(ValueError, match=f"id {name} of list"):
                f(good, gl, TAUS, bad)
        with pytest.raises(ValueError, match="query length"):
            f(np.ascontiguousarray(good[:, :10]), gl, TAUS, lists)
        with pytest.raises(ValueError, match="id lists"):
            f(good, gl, TAUS, lists[:2])
        with pytest.raises(TypeError):
            f(good, gl, [[1.0, 0.5]], lists)
        with pytest.raises(TypeError):
            f(good, None, TAUS, lists)
    EINVAL = asp._lib.AS_EINVAL
    ids = np.array([1, 2, 3, 4], dtype=np.int64)
    for offs in ([0, 3, 2, 4], [1, 2, 3, 4]):   # decreasing; not starting at 0
        st, out, _, _ = raw_scores(asp, aspace, gl, good, TAUS, ids, offs, fill=-5.0)
        assert st == EINVAL and "offsets" in asp._lib.last_error() and (out == -5.0).all()
        assert raw_search(asp, aspace, gl, good, TAUS, ids, offs, 5)[0] == EINVAL
    # a null taus with ntau > 0
    offs3 = np.array([0, 2, 3, 4], dtype=np.int64)
    out = np.full(8, -5.0)
    assert asp._L.as_score_lists_batch_taus(aspace._h, gl._h, good.ctypes.data, 3, d, None, 2, ids.ctypes.data, offs3.ctypes.data,
                                            out.ctypes.data, None, None) == EINVAL
    assert (out == -5.0).all()
    assert aspace.lists_sweep_counters() == before   # every one of them was refused before the lambda_q step: nothing was launched
    # taus = [], B == 0, empty lists
    assert aspace.search_batch_lists_taus(good, gl, [], lists) == [[], [], []]
    assert [r.shape for r in aspace.score_lists_batch_taus(good, gl, [], lists)] == [(0, 3), (0, 2), (0, 0)]
    assert aspace.score_lists_batch_taus(good, gl, [], np.array([[1, 2], [3, 4], [5, 6]])).shape == (3, 0, 2)
    none = np.empty((0, d))
    assert aspace.search_batch_lists_taus(none, gl, TAUS, []) == []
    assert aspace.score_lists_batch_taus(none, gl, TAUS, []) == []
    assert aspace.score_lists_batch_taus(none, gl, TAUS, np.empty((0, 3), dtype=np.int64)).shape == (0, 3, 3)
    now = aspace.lists_sweep_counters()
    assert now["lambda_steps"] == before["lambda_steps"] and now["score_launches"] == before["score_launches"]
    assert aspace.search_batch_lists_taus(good, gl, TAUS, [[], [], []]) == [[[], [], []]] * 3
    assert [r.shape for r in aspace.score_lists_batch_taus(good, gl, TAUS, [[], [], []])] == [(3, 0)] * 3
    now = aspace.lists_sweep_counters()
    assert now["lambda_steps"] == before["lambda_steps"] + 2 and now["score_launches"] == before["score_launches"]
    assert aspace.lists_counters() == single


def test_a_zero_lambda_query_is_skipped_and_its_neighbours_served():
    import pyarrowspace_amd as asp
    n, d = 800, 32
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
    for taus in ([0.62, 1.0, 0.0], [0.62, 1.0, 0.62]):   # (with a repeated tau: its copy leaves the block alone as well)
        st, out, lq, stt = raw_scores(asp, aspace, gl, Q, taus, ids, offs)
        assert st == 0 and stt.tolist() == [0, 0, ZL, 0] and lq[2] == 0.0 and (lq[[0, 1, 3]] != 0.0).all()
        assert np.isnan(out[3 * offs[2]:3 * offs[3]]).all()   # its block: left unwritten
        assert not np.isnan(out[:3 * offs[2]]).any() and not np.isnan(out[3 * offs[3]:]).any()
        st, hits, lq2, stt, ln = raw_search(asp, aspace, gl, Q, taus, ids, offs, 5)
        assert st == 0 and stt.tolist() == [0, 0, ZL, 0] and ln.tolist() == [[5] * 3, [3] * 3, [0] * 3, [5] * 3] and np.array_equal(lq, lq2)
        for j, tau in enumerate(taus):
            for i in (0, 1, 3):
                m = offs[i + 1] - offs[i]
                np.testing.assert_allclose(out[3 * offs[i] + j * m:3 * offs[i] + (j + 1) * m],
                                           aspace.score_items(np.ascontiguousarray(Q[i]), gl, tau, lists[i]), rtol=1e-12, atol=0.0)
                same_as_single(hits[i][j], aspace.search_subset(np.ascontiguousarray(Q[i]), gl, tau, lists[i]))
    st, _, _, stt = raw_scores(asp, aspace, gl, Q, TAUS, [], [0, 0, 0, 0, 0])   # empty lists still run the lambda_q step
    assert st == 0 and stt.tolist() == [0, 0, ZL, 0]
    for ls in (lists, [[], [], [], []]):
        with pytest.raises(asp.PanicException):
            aspace.search_batch_lists_taus(Q, gl, TAUS, ls)
        with pytest.raises(asp.PanicException):
            aspace.score_lists_batch_taus(Q, gl, TAUS, ls)


# ---------------------------------------------------------------- 8. other index modes
@pytest.mark.parametrize("extra", [{"lambda_mode": "feature", "metric": "cosine", "kernel": "rational"}, {"force_exact": True}],
                         ids=["feature", "force_exact"])
def test_feature_lambda_and_force_exact_indexes(extra):
    import pyarrowspace_amd as asp
    n, d = 800, 24
    X = clustered(n, d, nclust=8, seed=18)
    eps = calibrate_feature_eps(X, 6) if "lambda_mode" in extra else calibrate_eps(X, 6)
    aspace, gl = asp.ArrowSpaceBuilder.build(dict({"eps": eps, "k": 6, "topk": 8, "p": 2.0, "sigma": None}, **extra), X)
    rng = np.random.default_rng(19)
    Q, lqs = draw_queries(aspace, gl, X, rng, 4)
    lam = aspace.lambdas()
    lists = [rng.choice(n, m, replace=False) for m in (200, 5, 65, n)]
    check_sweep(aspace, gl, Q, TAUS, lists, lambda i, tau: np_scores(X, lam, lqs[i], Q[i], tau), 8, d)
    check_against_single(aspace, gl, Q, TAUS, lists)


# ---------------------------------------------------------------- 9. threads
def test_four_threads_on_one_space(swept):
    aspace, gl, Q, _, _, n = swept
    rng = np.random.default_rng(46)
    Qb = np.ascontiguousarray(Q[:12])
    lists = [rng.choice(n, m, replace=False) for m in (5, 64, 700, 1500, 1, 130, 4000, 33, 0, 250, 1025, 90)]
    taus = [1.0, 0.62, 0.0]
    sweeps = aspace.search_batch_lists_taus(Qb, gl, taus, lists)
    planes = aspace.score_lists_batch_taus(Qb, gl, taus, lists)
    rows = aspace.score_lists_batch(Qb, gl, 0.62, lists)
    singles = [aspace.search(np.ascontiguousarray(q), gl, 0.62) for q in Qb]
    errors = []

    def run(f):
        def body():
            try:
                for _ in range(6):
                    f()
            except BaseException as e:   # noqa: BLE001
                errors.append(e)
        return threading.Thread(target=body)

    def sweep():
        assert aspace.search_batch_lists_taus(Qb, gl, taus, lists) == sweeps

    def sweep_scores():
        got = aspace.score_lists_batch_taus(Qb, gl, taus, lists)
        assert all(np.array_equal(bits(g), bits(p)) for g, p in zip(got, planes))

    def single_tau():
        got = aspace.score_lists_batch(Qb, gl, 0.62, lists)
        assert all(np.array_equal(bits(g), bits(r)) for g, r in zip(got, rows))

    def search():
        assert [aspace.search(np.ascontiguousarray(q), gl, 0.62) for q in Qb] == singles

    th = [run(f) for f in (sweep, sweep_scores, single_tau, search)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]
