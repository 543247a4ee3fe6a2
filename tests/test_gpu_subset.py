"""GPU: filtered search -- ArrowSpace.subset / search_subset / score_items.  A subset restricts which items may be returned,
not the index: lambda_q and the items' lambdas are the ones `search` uses.  Expected values: the oracle's score of every item
restricted to the subset and ordered by (score descending, index ascending), or the same from numpy in fp64 over the items,
`aspace.lambdas()` and `aspace.query_lambda()` (gather, score and selection checked independently of the lambdas)."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

from conftest import assert_hits_match, calibrate_eps, calibrate_feature_eps, clustered
from test_gpu_parity import RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def atol_for(d):
    """fp64 dot error of unit-norm rows: a subset's scores at tau = 1 can sit near 0, where a relative bound means nothing."""
    return 16 * d * 2.0 ** -53


def same_as_single(sweep, single, tie=1e-12):
    """The subset's list against search()'s: the same indices in the same order except where two scores tie to `tie`
    relative, scores within `tie` relative."""
    assert len(sweep) == len(single), (sweep, single)
    gs = np.array([s for _, s in sweep])
    ws = np.array([s for _, s in single])
    np.testing.assert_allclose(gs, ws, rtol=tie, atol=0.0)
    for t, ((a, _), (b, _)) in enumerate(zip(sweep, single)):
        if a != b:
            tied = [u for u in range(len(ws)) if abs(ws[u] - ws[t]) <= tie * max(abs(ws[t]), 1e-300)]
            assert len(tied) > 1 and a in [single[u][0] for u in tied], (t, sweep, single)


def np_scores(X, lam, lq, q, tau):
    """SPEC S11 over every item, fp64: tau cos + (1 - tau) / (1 + |lambda_q - lambda_i|), cos = 0 for a zero row."""
    den = np.sqrt(np.einsum("ij,ij->i", X, X) * (q @ q))
    c = np.where(den > 0, (X @ q) / np.where(den > 0, den, 1.0), 0.0)
    return tau * c + (1.0 - tau) / (1.0 + np.abs(lq - lam))


def expected(all_scores, ids, topk):
    """The first min(topk, |S|) of the subset by (score descending, index ascending)."""
    u = np.unique(np.asarray(ids, dtype=np.int64))
    s = all_scores[u]
    order = np.lexsort((u, -s))[:topk]
    return [(int(u[t]), float(s[t])) for t in order]


def check_subset(aspace, gl, q, tau, subset, ids, all_scores, topk, d):
    got = aspace.search_subset(q, gl, tau, subset)
    want = expected(all_scores, ids, topk)
    uniq = set(np.unique(ids).tolist())
    assert len(got) == min(topk, len(uniq))
    assert all(i in uniq for i, _ in got), (got, sorted(uniq)[:20])
    assert_hits_match(got, want, all_scores, rtol=RTOL, atol=atol_for(d))
    return got


def subsets_of(n, rng):
    half = rng.choice(n, n // 2, replace=False)
    dup = np.concatenate([rng.integers(0, n, 40), rng.integers(0, n, 40)[:20], [n - 1, 0, n - 1]])
    dup = np.concatenate([dup, dup[:25]])
    rng.shuffle(dup)
    mask = rng.random(n) < 0.3
    return [("one percent", rng.choice(n, max(n // 100, 1), replace=False)), ("half", half), ("all", np.arange(n)),
            ("one id", np.array([int(rng.integers(0, n))])), ("ends", np.array([0, n - 1])), ("shuffled duplicates", dup),
            ("mask", mask)]


@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
@pytest.mark.parametrize("n,d,k,topk,metric,kernel", [(1200, 48, 10, 10, "l2", "gaussian"), (3000, 96, 25, 10, "cosine", "rational"),
                                                       (2000, 768, 25, 15, "l2", "gaussian"), (1500, 51, 8, 6, "l2", "gaussian")])
def test_subset_matches_oracle(oracle_lib, n, d, k, topk, metric, kernel, f32):
    """x64: the items as they are (fp64 rows kept; d = 51: rows that are not 16-byte aligned); x32: rounded through float32
    (the fp32 rows are the exact items, no fp64 copy)."""
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
    for name, ids in subs:
        u = np.flatnonzero(ids) if ids.dtype == np.bool_ else np.unique(ids)
        assert prepared[name].size == len(u) and np.array_equal(prepared[name].ids(), u)
    checked = 0
    for _ in range(3):
        q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        try:
            _, lq = ref.search(q, 1.0)
        except oracle_lib.ZeroLambda:
            continue
        checked += 1
        for tau in (1.0, 0.62, 0.0):
            sc = ref.scores(q, tau, lq)
            for name, ids in subs:
                idl = np.flatnonzero(ids) if ids.dtype == np.bool_ else ids
                check_subset(aspace, gl, q, tau, prepared[name], idl, sc, topk, d)
            # the ad-hoc forms: an array, a list, a mask
            check_subset(aspace, gl, q, tau, subs[5][1], subs[5][1], sc, topk, d)
            check_subset(aspace, gl, q, tau, subs[4][1].tolist(), subs[4][1], sc, topk, d)
            check_subset(aspace, gl, q, tau, subs[6][1], np.flatnonzero(subs[6][1]), sc, topk, d)
    assert checked > 0


def raw_search_subset(asp, aspace, gl, q, tau, sub, cap):
    idx = np.empty(cap, dtype=np.int64)
    sc = np.empty(cap, dtype=np.float64)
    ln, lq = C.c_int64(-1), C.c_double(-1.0)
    st = asp._L.as_search_subset(aspace._h, gl._h, q.ctypes.data, q.shape[0], tau, sub._h, idx.ctypes.data, sc.ctypes.data, C.byref(ln),
                                 C.byref(lq))
    return st, list(zip(idx[:max(ln.value, 0)].tolist(), sc[:max(ln.value, 0)].tolist())), lq.value


@pytest.mark.parametrize("f32", [False, True], ids=["x64", "x32"])
def test_full_subset_is_search_and_score_items_reproduces_it(oracle_lib, f32):
    import pyarrowspace_amd as asp
    n, d, k, topk = 2500, 200, 12, 20
    X = clustered(n, d, nclust=24, seed=3)
    if f32:
        X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
    gp = {"eps": calibrate_eps(X, k), "k": k, "topk": topk, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    ref = oracle_lib.OracleIndex(X, gp)
    full = aspace.subset(np.ones(n, dtype=bool))
    assert full.size == n
    rng = np.random.default_rng(8)
    checked = 0
    for _ in range(4):
        q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        try:
            _, lq_ref = ref.search(q, 1.0)
        except oracle_lib.ZeroLambda:
            continue
        checked += 1
        for tau in (1.0, 0.62, 0.0):
            single = aspace.search(q, gl, tau)
            same_as_single(aspace.search_subset(q, gl, tau, full), single)
            st, hits, lq = raw_search_subset(asp, aspace, gl, q, tau, full, topk)
            assert st == 0 and lq == aspace.query_lambda(q, gl)
            same_as_single(hits, single)
            # score_items: the scores search gives its hits, and the oracle's scores in the caller's order with duplicates
            ids = [i for i, _ in single]
            np.testing.assert_allclose(aspace.score_items(q, gl, tau, ids), [s for _, s in single], rtol=1e-12, atol=0.0)
            mixed = np.concatenate([rng.integers(0, n, 300), ids[::-1], ids, [0, n - 1, 0]])
            got = aspace.score_items(q, gl, tau, mixed)
            assert got.dtype == np.float64 and got.shape == mixed.shape
            np.testing.assert_allclose(got, ref.scores(q, tau, lq_ref)[mixed], rtol=RTOL, atol=atol_for(d))
            assert np.array_equal(got[-3], got[-1])
    assert checked > 0
    assert aspace.score_items(np.ascontiguousarray(X[0]), gl, 0.5, []).shape == (0,)


def test_exact_ties_come_back_in_index_order():
    import pyarrowspace_amd as asp
    n, d = 1000, 40
    X = clustered(n, d, nclust=8, seed=6)
    X[500] = X[10]
    X[900] = X[10]
    gp = {"eps": calibrate_eps(X, 8), "k": 8, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    q = np.ascontiguousarray(X[10] * 1.01)
    rest = [i for i in range(999, -1, -7) if i not in (10, 500, 900)]
    got = aspace.search_subset(q, gl, 1.0, [900, 500] + rest + [10])
    assert [i for i, _ in got[:3]] == [10, 500, 900]
    assert got[0][1] == got[1][1] == got[2][1]
    assert got[3][1] < got[2][1]
    sc = aspace.score_items(q, gl, 1.0, [900, 10, 500])
    assert sc[0] == sc[1] == sc[2] == got[0][1]


@pytest.fixture(scope="module")
def big():
    """n = 70 000: more than one block and more than one round of every selection kernel."""
    import pyarrowspace_amd as asp
    n, d = 70_000, 32
    X = clustered(n, d, nclust=64, seed=12)
    gp = {"eps": calibrate_eps(X, 4), "k": 4, "topk": 3, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    return X, aspace, gl, aspace.lambdas()


@pytest.mark.parametrize("which", ["all", "65537", "duplicates"])
def test_many_blocks_and_rounds(big, which):
    X, aspace, gl, lam = big
    n, d = X.shape
    rng = np.random.default_rng(13)
    ids = {"all": np.arange(n), "65537": rng.choice(n, 65537, replace=False),
           "duplicates": rng.choice(n, 300, replace=False)[rng.integers(0, 300, 70_000)]}[which]
    sub = aspace.subset(ids)
    assert sub.size == len(np.unique(ids))
    checked = 0
    for r in range(3):
        q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        lq = aspace.query_lambda(q, gl)
        if lq == 0.0:
            continue
        checked += 1
        for tau in (1.0, 0.62, 0.0):
            sc = np_scores(X, lam, lq, q, tau)
            check_subset(aspace, gl, q, tau, sub, ids, sc, 3, d)
            if which != "all":
                # the same ids scored one by one, the caller's order and duplicates kept
                np.testing.assert_allclose(aspace.score_items(q, gl, tau, ids), sc[ids], rtol=RTOL, atol=atol_for(d))
    assert checked > 0


def test_a_run_of_equal_scores_across_the_threshold_of_the_radix_select():
    """200 rows that are 0.5 x row 20: their cosines against any query are row 20's bit for bit (a power of two scales the dot and
    the norm exactly).  At tau = 1 they tie at the top of more than 1024 scores: the selection's threshold falls inside the run,
    and the lowest positions must win."""
    import pyarrowspace_amd as asp
    n, d = 4000, 32
    X = clustered(n, d, nclust=16, seed=22)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}   # (before the copies: their distances are 0)
    X[1000:1200] = 0.5 * X[20]
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    q = np.ascontiguousarray(X[20] * 1.01)
    assert aspace.query_lambda(q, gl) != 0.0
    got = aspace.search_subset(q, gl, 1.0, np.arange(n))
    assert [i for i, _ in got] == [20, 1000, 1001, 1002, 1003]
    assert len({s for _, s in got}) == 1
    got = aspace.search_subset(q, gl, 1.0, np.arange(n - 1, 499, -1))
    assert [i for i, _ in got] == [1000, 1001, 1002, 1003, 1004]
    assert len({s for _, s in got}) == 1


WIDE_RUNS = [(3800, 4400, 300), (3900, 5000, 1024)]


def wide_tie_run(first, last, topk):
    """5000 items, ids first .. last - 1 copies of 0.5 x row 20, the query 1.01 x row 20: at tau = 1 the winners are 20 and the
    run's first topk - 1.  The threshold lies inside the run AND the run crosses position 4096, where digit 6 of the key (bits
    12 .. 23 of ~position) changes: that pass of the radix select, not only the last, has to pick a digit by rank.  600 ties fit
    the 1024 entries the final sort ranks, so a threshold found too low would be put right there; 1100 ties with topk = 1024 do
    not fit, and every entry the collection drops is missed."""
    import pyarrowspace_amd as asp
    n, d = 5000, 32
    X = clustered(n, d, nclust=16, seed=22)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": topk, "p": 2.0, "sigma": None}   # (before the copies: their distances are 0)
    X[first:last] = 0.5 * X[20]
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    q = np.ascontiguousarray(X[20] * 1.01)
    assert aspace.query_lambda(q, gl) != 0.0
    return aspace, gl, X, q, [20] + list(range(first, first + topk - 1))


@pytest.mark.parametrize("first,last,topk", WIDE_RUNS)
def test_a_run_of_equal_scores_that_reaches_the_position_digits(first, last, topk):
    aspace, gl, X, q, winners = wide_tie_run(first, last, topk)
    n = X.shape[0]
    every = np.arange(n)
    s = aspace.score_items(q, gl, 1.0, [20, first, 4095, 4096, last - 1])
    assert len(set(s.view(np.uint64).tolist())) == 1 and s[0] > np.delete(aspace.score_items(q, gl, 1.0, every), [20] + list(range(first, last))).max()
    forms = {"search_subset": aspace.search_subset(q, gl, 1.0, every),
             "search_batch_lists": aspace.search_batch_lists(q[None, :], gl, 1.0, [every])[0],
             "search_batch_lists, descending": aspace.search_batch_lists(q[None, :], gl, 1.0, [every[::-1].copy()])[0],   # the winners come last
             "search_fused": aspace.search_fused(q[None, :], gl, 1.0, weights=[1.0], subset=every)}
    for form, got in forms.items():
        assert [i for i, _ in got] == winners, form
        assert len({np.float64(v).view(np.uint64).item() for _, v in got}) == 1, form
    # without the head and the run's first 200 the run starts at position first - 1 of the subset: it crosses 4096 again, and
    # the next 300 ids win
    if last - first - 200 >= topk:
        got = aspace.search_subset(q, gl, 1.0, np.delete(every, [20] + list(range(first, first + 200))))
        assert [i for i, _ in got] == list(range(first + 200, first + 200 + topk)) and len({v for _, v in got}) == 1


@pytest.mark.parametrize("topk", [1024, 1])
def test_topk_edges(topk):
    import pyarrowspace_amd as asp
    n, d = 5000, 32
    X = clustered(n, d, nclust=16, seed=15)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": topk, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    lam = aspace.lambdas()
    rng = np.random.default_rng(16)
    q = np.ascontiguousarray(X[77] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
    lq = aspace.query_lambda(q, gl)
    assert lq != 0.0
    for m in (3000, 700):
        ids = rng.choice(n, m, replace=False)
        for tau in (1.0, 0.62):
            got = check_subset(aspace, gl, q, tau, ids, ids, np_scores(X, lam, lq, q, tau), topk, d)
            assert len(got) == min(topk, m)


def test_zero_norm_row_scores_its_lambda_term():
    import pyarrowspace_amd as asp
    n, d = 900, 24
    X = clustered(n, d, nclust=8, seed=17)
    X[5] = 0.0
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 12, "p": 2.0, "sigma": None, "metric": "l2"}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    lam = aspace.lambdas()
    q = np.ascontiguousarray(X[40] * 1.01)
    lq = aspace.query_lambda(q, gl)
    assert lq != 0.0
    tau = 0.62
    sc = np_scores(X, lam, lq, q, tau)
    order = np.argsort(-sc)
    ids = np.concatenate([order[:4], order[-4:], [5]])   # the zero row between rows of positive and of negative cosine
    got = check_subset(aspace, gl, q, tau, ids, ids, sc, 12, d)
    at = [i for i, _ in got].index(5)
    assert got[at][1] == pytest.approx((1.0 - tau) / (1.0 + abs(lq - lam[5])), rel=1e-15)
    assert aspace.score_items(q, gl, tau, [5])[0] == got[at][1]


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
    checked = 0
    for _ in range(3):
        q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        lq = aspace.query_lambda(q, gl)
        if lq == 0.0:
            continue
        checked += 1
        for tau in (1.0, 0.62, 0.0):
            sc = np_scores(X, lam, lq, q, tau)
            check_subset(aspace, gl, q, tau, ids, ids, sc, 8, d)
            same_as_single(aspace.search_subset(q, gl, tau, np.arange(n)), aspace.search(q, gl, tau))
    assert checked > 0


def test_one_subset_over_many_queries_and_threads():
    import pyarrowspace_amd as asp
    n, d = 4000, 64
    X = clustered(n, d, nclust=32, seed=20)
    gp = {"eps": calibrate_eps(X, 10), "k": 10, "topk": 10, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(21)
    ids = rng.choice(n, 1500, replace=False)
    sub = aspace.subset(ids)
    Q = []
    while len(Q) < 20:
        q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        if aspace.query_lambda(q, gl) != 0.0:
            Q.append(q)
    serial = [aspace.search_subset(q, gl, 0.62, sub) for q in Q]
    assert serial == [aspace.search_subset(q, gl, 0.62, ids) for q in Q]
    single = [aspace.search(q, gl, 0.62) for q in Q]
    errors = []

    def filtered():
        try:
            for _ in range(3):
                for q, want in zip(Q, serial):
                    assert aspace.search_subset(q, gl, 0.62, sub) == want
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    def plain():
        try:
            for _ in range(3):
                for q, want in zip(Q, single):
                    assert aspace.search(q, gl, 0.62) == want
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=filtered), threading.Thread(target=filtered), threading.Thread(target=plain)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]


def test_errors():
    import pyarrowspace_amd as asp
    n, d = 800, 32
    X = clustered(n, d, nclust=8, seed=4)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    other, gl2 = asp.ArrowSpaceBuilder.build(gp, X[:400].copy())
    near = np.ascontiguousarray(X[3] * 1.01)
    far = np.ascontiguousarray(np.full(d, 50.0))   # no item within eps: lambda_q == 0
    with pytest.raises(asp.PanicException):
        aspace.search(far, gl, 1.0)
    assert aspace.search(near, gl, 0.62)
    for bad in ([0, n], [-1, 3]):
        with pytest.raises(ValueError, match="id"):
            aspace.subset(bad)
        with pytest.raises(ValueError):
            aspace.search_subset(near, gl, 0.62, bad)
        with pytest.raises(ValueError):
            aspace.score_items(near, gl, 0.62, bad)
    with pytest.raises(TypeError):
        aspace.subset(np.array([1.0, 2.0]))
    with pytest.raises(TypeError):
        aspace.score_items(near, gl, 0.62, [1.5])
    with pytest.raises(ValueError):
        aspace.subset(np.ones(n - 1, dtype=bool))
    with pytest.raises(ValueError):
        asp.ItemSubset()
    sub = aspace.subset([1, 2, 3])
    with pytest.raises(ValueError, match="another space"):
        other.search_subset(np.ascontiguousarray(X[3] * 1.01), gl2, 0.62, sub)
    with pytest.raises(ValueError, match="query length"):
        aspace.search_subset(np.ascontiguousarray(near[:10]), gl, 0.62, sub)
    with pytest.raises(ValueError, match="query length"):
        aspace.score_items(np.ascontiguousarray(near[:10]), gl, 0.62, [1, 2])
    with pytest.raises(TypeError):
        aspace.search_subset(near.astype(np.float32), gl, 0.62, sub)
    with pytest.raises(TypeError):
        aspace.score_items(near.astype(np.float32), gl, 0.62, [1, 2])
    with pytest.raises(TypeError):
        aspace.search_subset(near, None, 0.62, sub)
    with pytest.raises(ValueError, match="tau"):
        aspace.search_subset(near, gl, float("nan"), sub)
    with pytest.raises(ValueError, match="tau"):
        aspace.score_items(near, gl, float("inf"), [1, 2])
    empty = aspace.subset([])
    assert empty.size == 0 and empty.ids().shape == (0,)
    for s in (sub, empty, [], [4, 5]):
        with pytest.raises(asp.PanicException):
            aspace.search_subset(far, gl, 0.62, s)
    with pytest.raises(asp.PanicException):
        aspace.score_items(far, gl, 0.62, [1, 2])
    with pytest.raises(asp.PanicException):
        aspace.score_items(far, gl, 0.62, [])
    assert aspace.search_subset(near, gl, 0.62, empty) == []
    assert aspace.search_subset(near, gl, 0.62, []) == []
    assert aspace.search_subset(near, gl, 0.62, np.zeros(n, dtype=bool)) == []
    assert [i for i, _ in aspace.search_subset(near, gl, 1.0, sub)][0] == 3
