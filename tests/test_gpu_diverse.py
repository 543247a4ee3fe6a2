"""GPU: diversified search -- ArrowSpace.search_diverse / search_batch_diverse (greedy maximal marginal relevance over the hit list
of the ordinary route).  Every expected value comes from tests/diverse_ref.py on the pool that the ordinary route
(`search`, `search_subset`, `search_batch`, `search_batch_subset`) returns on the GPU in the same test, so only the new code is
under test.  tests/test_diverse_inputs.py shows that on these inputs the stepwise check admits the reference's path only."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

import diverse_ref as dr
from conftest import calibrate_eps, calibrate_feature_eps, clustered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TAU = 0.62
_built = {}
TOTAL = {"steps": 0, "ambiguous": 0}   # over every stepwise check of the module


class Index:
    """One index with what the checks need: the items, their squared norms and a cache of item-item cosines."""

    def __init__(self, X, gp):
        import pyarrowspace_amd as asp
        self.asp, self.X, self.gp = asp, X, gp
        self.aspace, self.gl = asp.ArrowSpaceBuilder.build(gp, X)
        self.n, self.d = X.shape
        self.n64 = np.einsum("ij,ij->i", X, X)
        self.cache = dr.new_cache(self.n)
        self.tol = dr.tol_for(self.d)

    def queries(self, rng, count):
        return dr.queries_of(self.X, rng, count, lambda q: self.aspace.query_lambda(q, self.gl) != 0.0)


def index(name):
    """One index per shape for the whole module."""
    if name not in _built:
        _built[name] = Index(*dr.shape_items(name))
    return _built[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def verify(ix, res, pool, n, delta):
    """A list [(index, score, margin)] against the pool [(index, score)] it was made from: length, first pick, no repeats, the
    pool's score bits, then the stepwise check."""
    ids = [i for i, _ in pool]
    s = [v for _, v in pool]
    P = len(pool)
    assert len(res) == min(n, P), (len(res), n, P)
    if not res:
        return
    assert res[0][0] == ids[0]
    got = [i for i, _, _ in res]
    assert len(set(got)) == len(got)
    pos = {i: p for p, i in enumerate(ids)}
    assert all(i in pos for i in got)
    assert bits([v for _, v, _ in res]) == bits([s[pos[i]] for i in got])
    G = dr.pool_gram(ix.X, ix.n64, ids, ix.cache)
    TOTAL["ambiguous"] += dr.check_steps(res, ix.X, ix.n64, ids, s, delta, ix.tol, G=G)
    TOTAL["steps"] += len(res)


def counters(ix):
    out = (C.c_int64 * 5)()
    assert ix.asp._L.as_diverse_counters(ix.aspace._h, out, 5) == 0
    return list(out)


def batch_pools(ix, Q, tau, sub):
    """The lists of `search_batch` / `search_batch_subset` for Q with the status of every query (the C ABI: the Python methods
    panic when one query's lambda_q is 0)."""
    L, aspace, gl = ix.asp._L, ix.aspace, ix.gl
    b = Q.shape[0]
    kk = min(int(gl.graph_params["topk"]), ix.n, ix.n if sub is None else sub.size)
    idx = np.empty((b, kk), dtype=np.int64)
    sc = np.empty((b, kk), dtype=np.float64)
    ln = np.zeros(b, dtype=np.int64)
    st = np.zeros(b, dtype=np.int32)
    if sub is None:
        rc = L.as_search_batch(aspace._h, gl._h, Q.ctypes.data, b, Q.shape[1], tau, idx.ctypes.data, sc.ctypes.data, ln.ctypes.data, None,
                               st.ctypes.data)
    else:
        rc = L.as_search_subset_batch(aspace._h, gl._h, Q.ctypes.data, b, Q.shape[1], tau, sub._h, idx.ctypes.data, sc.ctypes.data,
                                      ln.ctypes.data, None, st.ctypes.data)
    assert rc == 0, ix.asp._lib.last_error()
    pools = [list(zip(idx[i, :ln[i]].tolist(), sc[i, :ln[i]].tolist())) if st[i] == 0 else [] for i in range(b)]
    return pools, st.tolist()


@pytest.mark.parametrize("name", list(dr.SHAPES))
def test_diversity_zero_returns_the_head_of_the_pool(name):
    ix = index(name)
    q = ix.queries(np.random.default_rng(3), 1)[0]
    pool = ix.aspace.search(q, ix.gl, TAU)
    P = len(pool)
    assert P == min(ix.gp["topk"], ix.n)
    for n in (1, 2, P - 1, P, P + 5):
        res = ix.aspace.search_diverse(q, ix.gl, TAU, n, 0.0, with_margins=True)
        k = min(n, P)
        assert [i for i, _, _ in res] == [i for i, _ in pool[:k]], n
        assert bits([v for _, v, _ in res]) == bits([v for _, v in pool[:k]]), n
        assert [m for _, _, m in res] == [v for _, v in pool[:k]], n   # (1 - 0) s - 0 r
        assert ix.aspace.search_diverse(q, ix.gl, TAU, n, 0.0) == pool[:k]


@pytest.mark.parametrize("name", list(dr.SHAPES))
def test_stepwise_check_over_diversities_and_lengths(name):
    ix = index(name)
    Q = ix.queries(np.random.default_rng(5), dr.NQ)
    moved = 0
    for q in Q:
        pool = ix.aspace.search(q, ix.gl, TAU)
        P = len(pool)
        for delta in dr.DELTAS:
            for n in sorted({1, 2, min(16, P), P}):
                res = ix.aspace.search_diverse(q, ix.gl, TAU, n, delta, with_margins=True)
                verify(ix, res, pool, n, delta)
                plain = ix.aspace.search_diverse(q, ix.gl, TAU, n, delta)
                assert plain == [(i, v) for i, v, _ in res]
                moved += [i for i, _ in plain] != [i for i, _ in pool[:len(plain)]]
    assert moved >= len(Q) * len(dr.DELTAS)   # (the CPU check of these inputs: every case with n >= 16 reorders)


def hand_index():
    """A small index with hand-placed rows: 5 is zero, 7 is the exact negation of 6, 9 .. 11 are three copies of one row."""
    if "hand" not in _built:
        n, d = 900, 24
        X = clustered(n, d, nclust=8, seed=23)
        X[5] = 0.0
        X[7] = -X[6]
        X[10] = X[9]
        X[11] = X[9]
        gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 12, "p": 2.0, "sigma": None, "metric": "l2"}
        _built["hand"] = Index(X, gp)
    return _built["hand"]


def test_subsets_that_force_the_pool():
    ix = hand_index()
    aspace, gl, X = ix.aspace, ix.gl, ix.X
    rng = np.random.default_rng(29)
    others = [int(i) for i in rng.choice(np.arange(20, ix.n), 6, replace=False)]
    q = np.ascontiguousarray(X[40] * 1.01)
    assert aspace.query_lambda(q, gl) != 0.0
    # |S| = 1 and 2: P < topk, n larger than the pool
    for S in ([40], [40, 41]):
        pool = aspace.search_subset(q, gl, TAU, S)
        assert len(pool) == len(S) < ix.gp["topk"]
        for n in (1, 2, 5):
            verify(ix, aspace.search_diverse(q, gl, TAU, n, 0.5, subset=S, with_margins=True), pool, n, 0.5)
    # a prepared handle and an ad-hoc list are the same subset
    sub = aspace.subset(others)
    assert aspace.search_diverse(q, gl, TAU, 4, 0.5, subset=sub) == aspace.search_diverse(q, gl, TAU, 4, 0.5, subset=others)
    # a zero row: its cosine with everything is 0, its margin (1 - delta) s whenever it is picked
    S = [5] + others
    pool = aspace.search_subset(q, gl, TAU, S)
    for delta in (0.5, 1.0):
        res = aspace.search_diverse(q, gl, TAU, len(S), delta, subset=S, with_margins=True)
        verify(ix, res, pool, len(S), delta)
        at = [i for i, _, _ in res].index(5)
        assert res[at][2] == pytest.approx((1.0 - delta) * res[at][1], abs=ix.tol)
    # a row and its exact negation: g = -1, the margin gains delta
    q6 = np.ascontiguousarray(X[6] * 1.01)
    assert aspace.query_lambda(q6, gl) != 0.0
    for S in ([6, 7], [6, 7] + others):
        pool = aspace.search_subset(q6, gl, 1.0, S)
        assert pool[0][0] == 6
        for delta in (0.3, 0.9):
            res = aspace.search_diverse(q6, gl, 1.0, len(S), delta, subset=S, with_margins=True)
            verify(ix, res, pool, len(S), delta)
            assert res[0][0] == 6
            # with m_7 = (1 - delta) (-1) + delta = 2 delta - 1 against (1 - 2 delta) s_o for a row of cosine s_o with 6, the
            # negation comes second among other rows once delta > 1 / 2
            if len(S) == 2 or delta == 0.9:
                assert res[1][0] == 7
                assert res[1][2] == pytest.approx((1.0 - delta) * res[1][1] + delta, abs=ix.tol)
    # three copies of one row (tau = 1: identical rows, identical scores): the first copy picked is the lowest index, and no
    # copy is picked before a row whose reference margin exceeds its own by more than tol (the stepwise check)
    q9 = np.ascontiguousarray(X[9] * 1.01)
    assert aspace.query_lambda(q9, gl) != 0.0
    S = [11, 10, 9] + others
    pool = aspace.search_subset(q9, gl, 1.0, S)
    assert [i for i, _ in pool[:3]] == [9, 10, 11] and len({v for _, v in pool[:3]}) == 1
    for delta in (0.3, 0.5, 0.9):
        res = aspace.search_diverse(q9, gl, 1.0, len(S), delta, subset=S, with_margins=True)
        verify(ix, res, pool, len(S), delta)
        copies = [i for i, _, _ in res if i in (9, 10, 11)]
        assert copies[0] == 9 and sorted(copies) == [9, 10, 11]


@pytest.mark.parametrize("nb", [1, 2, 33, 65])
@pytest.mark.parametrize("name", ["1200x48", "300x4100"])
def test_batched_forms(name, nb):
    ix = index(name)
    asp, aspace, gl = ix.asp, ix.aspace, ix.gl
    rng = np.random.default_rng(200 + nb)
    Q = np.stack(ix.queries(rng, nb))
    zero_at = 1 if nb >= 2 else None
    if zero_at is not None:
        Q[zero_at] = 50.0   # no item within eps: lambda_q == 0
    half = aspace.subset(np.sort(rng.choice(ix.n, ix.n // 2, replace=False)))
    n, delta = 16, 0.5
    for sub in (None, half):
        pools, st = batch_pools(ix, Q, TAU, sub)
        assert [i for i, v in enumerate(st) if v != 0] == ([] if zero_at is None else [zero_at])
        got = aspace.search_batch_diverse(Q, gl, TAU, n, delta, subset=sub, with_margins=True)
        assert len(got) == nb
        for i in range(nb):
            if i == zero_at:
                assert got[i] == []
            else:
                verify(ix, got[i], pools[i], n, delta)
        assert aspace.search_batch_diverse(Q, gl, TAU, n, delta, subset=sub) == [[(i, v) for i, v, _ in g] for g in got]
        # the status of every query at the C ABI
        kk = min(ix.gp["topk"], ix.n if sub is None else sub.size)
        nn = min(n, kk)
        idx = np.full((nb, nn), -1, dtype=np.int64)
        sc = np.zeros((nb, nn))
        ln = np.full(nb, -1, dtype=np.int64)
        lq = np.full(nb, -1.0)
        st2 = np.full(nb, 9, dtype=np.int32)
        assert asp._L.as_search_diverse_batch(aspace._h, gl._h, Q.ctypes.data, nb, ix.d, TAU, n, delta, None if sub is None else sub._h,
                                              idx.ctypes.data, sc.ctypes.data, None, ln.ctypes.data, lq.ctypes.data, st2.ctypes.data) == 0
        assert st2.tolist() == st and ln.tolist() == [len(g) for g in got]
        assert all((lq[i] == 0.0) == (i == zero_at) for i in range(nb))
        assert [idx[i, :ln[i]].tolist() for i in range(nb)] == [[j for j, _, _ in g] for g in got]
        # the chunking never shows
        try:
            for chunk in (1, 7):
                assert asp._L.as_set_tuning(b"diverse_chunk", chunk) == 0
                c0 = counters(ix)
                again = aspace.search_batch_diverse(Q, gl, TAU, n, delta, subset=sub, with_margins=True)
                c1 = counters(ix)
                assert again == got
                assert all(bits([m for _, _, m in a]) == bits([m for _, _, m in g]) for a, g in zip(again, got))
                assert all(bits([v for _, v, _ in a]) == bits([v for _, v, _ in g]) for a, g in zip(again, got))
                # a chunk that holds the zero-lambda query alone launches nothing
                assert c1[1] - c0[1] == -(-nb // chunk) - (1 if chunk == 1 and zero_at is not None else 0)
        finally:
            assert asp._L.as_set_tuning(b"diverse_chunk", 0) == 0


def test_determinism_and_threads():
    ix = index("700x768f32")
    aspace, gl = ix.aspace, ix.gl
    Q = ix.queries(np.random.default_rng(31), 8)
    n, delta = 16, 0.5
    serial = [aspace.search_diverse(q, gl, TAU, n, delta, with_margins=True) for q in Q]
    assert [aspace.search_diverse(q, gl, TAU, n, delta, with_margins=True) for q in Q] == serial
    batch = aspace.search_batch_diverse(np.stack(Q), gl, TAU, n, delta, with_margins=True)
    assert aspace.search_batch_diverse(np.stack(Q), gl, TAU, n, delta, with_margins=True) == batch
    whole = aspace.search_diverse(Q[0], gl, TAU, 257, 0.9, with_margins=True)
    assert aspace.search_diverse(Q[0], gl, TAU, 257, 0.9, with_margins=True) == whole
    errors = []

    def run():
        try:
            for q, w in zip(Q, serial):
                assert aspace.search_diverse(q, gl, TAU, n, delta, with_margins=True) == w
            assert aspace.search_batch_diverse(np.stack(Q), gl, TAU, n, delta, with_margins=True) == batch
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=run) for _ in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]


def test_errors_on_a_live_space():
    ix = index("1200x48")
    asp, aspace, gl, X, d = ix.asp, ix.aspace, ix.gl, ix.X, ix.d
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    near = np.ascontiguousarray(X[3] * 1.01)
    far = np.ascontiguousarray(np.full(d, 50.0))
    Qn = np.stack([near, near * 1.01])
    assert aspace.query_lambda(near, gl) != 0.0
    other, gl2 = asp.ArrowSpaceBuilder.build(ix.gp, X[:400].copy())
    sub = aspace.subset([1, 2, 3])
    idx = np.full(64, -1, dtype=np.int64)
    sc = np.zeros(64)
    ln = C.c_int64(-1)
    st = np.zeros(2, dtype=np.int32)
    ln2 = np.zeros(2, dtype=np.int64)
    # the C ABI refuses n and the diversity itself, before anything is launched
    for n, delta in ((0, 0.5), (-1, 0.5), (4, -0.1), (4, 1.1), (4, float("nan"))):
        c0 = counters(ix)
        assert L.as_search_diverse(aspace._h, gl._h, near.ctypes.data, d, TAU, n, delta, None, idx.ctypes.data, sc.ctypes.data, None,
                                   C.byref(ln), None) == EINVAL
        assert ("n must be" if n < 1 else "diversity must") in asp._lib.last_error()
        assert L.as_search_diverse_batch(aspace._h, gl._h, Qn.ctypes.data, 2, d, TAU, n, delta, None, idx.ctypes.data, sc.ctypes.data, None,
                                         ln2.ctypes.data, None, st.ctypes.data) == EINVAL
        assert counters(ix) == c0 and ln.value == 0
        with pytest.raises(ValueError):
            aspace.search_diverse(near, gl, TAU, n, delta)
        with pytest.raises(ValueError):
            aspace.search_batch_diverse(Qn, gl, TAU, n, delta)
    # the filtered forms' checks and messages
    c0 = counters(ix)
    with pytest.raises(ValueError, match="query length"):
        aspace.search_diverse(np.ascontiguousarray(near[:10]), gl, TAU, 4, 0.5)
    with pytest.raises(ValueError, match="query length"):
        aspace.search_batch_diverse(np.ascontiguousarray(Qn[:, :10]), gl, TAU, 4, 0.5, subset=sub)
    with pytest.raises(ValueError, match="tau"):
        aspace.search_diverse(near, gl, float("inf"), 4, 0.5)
    with pytest.raises(ValueError, match="tau"):
        aspace.search_batch_diverse(Qn, gl, float("inf"), 4, 0.5)
    with pytest.raises(ValueError, match="another space"):
        other.search_diverse(np.ascontiguousarray(X[3] * 1.01), gl2, TAU, 4, 0.5, subset=sub)
    with pytest.raises(ValueError, match="another space"):
        other.search_batch_diverse(Qn, gl2, TAU, 4, 0.5, subset=sub)
    with pytest.raises(TypeError):
        aspace.search_diverse(near.astype(np.float32), gl, TAU, 4, 0.5)
    assert counters(ix) == c0
    # lambda_q == 0: the single form panics as `search`, whatever the subset; the batched form serves the others
    with pytest.raises(asp.PanicException):
        aspace.search(far, gl, TAU)
    for s in (None, sub, []):
        with pytest.raises(asp.PanicException):
            aspace.search_diverse(far, gl, TAU, 4, 0.5, subset=s)
    got = aspace.search_batch_diverse(np.stack([near, far, near]), gl, TAU, 4, 0.5)
    assert got[1] == [] and len(got[0]) == 4 and [i for i, _ in got[0]] == [i for i, _ in got[2]]
    # an empty subset: an empty answer, but the pool step runs; B == 0 launches nothing
    c0 = counters(ix)
    assert aspace.search_diverse(near, gl, TAU, 4, 0.5, subset=[]) == []
    assert aspace.search_batch_diverse(Qn, gl, TAU, 4, 0.5, subset=[]) == [[], []]
    c1 = counters(ix)
    assert c1[4] - c0[4] == 2 and c1[0] - c0[0] == 2 and c1[1] == c0[1]
    assert aspace.search_batch_diverse(np.empty((0, d)), gl, TAU, 4, 0.5) == []
    c2 = counters(ix)
    assert c2[1] == c1[1] and c2[4] == c1[4]


def test_feature_lambda_index():
    if "feature" not in _built:
        n, d = 800, 24
        X = clustered(n, d, nclust=8, seed=18)
        gp = {"eps": calibrate_feature_eps(X, 6), "k": 6, "topk": 32, "p": 2.0, "sigma": None, "metric": "cosine", "kernel": "rational",
              "lambda_mode": "feature"}
        _built["feature"] = Index(X, gp)
    ix = _built["feature"]
    assert ix.gl.lambda_mode == "feature"
    Q = ix.queries(np.random.default_rng(19), 3)
    sub = ix.aspace.subset(np.arange(0, ix.n, 3))
    for q in Q:
        for s, pool in ((None, ix.aspace.search(q, ix.gl, TAU)), (sub, ix.aspace.search_subset(q, ix.gl, TAU, sub))):
            for n in (4, len(pool)):
                verify(ix, ix.aspace.search_diverse(q, ix.gl, TAU, n, 0.5, subset=s, with_margins=True), pool, n, 0.5)
    pools, st = batch_pools(ix, np.stack(Q), TAU, None)
    for g, pool in zip(ix.aspace.search_batch_diverse(np.stack(Q), ix.gl, TAU, 8, 0.9, with_margins=True), pools):
        verify(ix, g, pool, 8, 0.9)


def test_counters_of_a_hand_counted_call():
    ix = index("1200x48")
    asp, aspace, gl = ix.asp, ix.aspace, ix.gl
    Q = ix.queries(np.random.default_rng(37), 3)
    P = len(aspace.search(Q[0], gl, TAU))
    assert P == 64
    c0 = counters(ix)
    assert len(aspace.search_diverse(Q[0], gl, TAU, 5, 0.5)) == 5
    c1 = counters(ix)
    # steps 1 .. 4 form 63 + 62 + 61 + 60 cosines; step 0 forms none
    assert [a - b for a, b in zip(c1, c0)] == [1, 1, 5, 63 + 62 + 61 + 60, 1]
    assert aspace.diverse_counters() == dict(zip(("calls", "launches", "picks", "dots", "pool_steps"), c1))
    assert len(aspace.search_diverse(Q[0], gl, TAU, 1, 0.5)) == 1   # one pick: no cosine at all
    c2 = counters(ix)
    assert [a - b for a, b in zip(c2, c1)] == [1, 1, 1, 0, 1]
    got = aspace.search_batch_diverse(np.stack(Q), gl, TAU, 3, 0.5)
    c3 = counters(ix)
    assert [len(g) for g in got] == [3, 3, 3]
    assert [a - b for a, b in zip(c3, c2)] == [1, 1, 9, 3 * (63 + 62), 1]   # one chunk, ONE batched pool step
    # n beyond the pool: the whole pool, P (P - 1) / 2 cosines
    assert len(aspace.search_diverse(Q[1], gl, TAU, P + 5, 0.5)) == P
    c4 = counters(ix)
    assert [a - b for a, b in zip(c4, c3)] == [1, 1, P, P * (P - 1) // 2, 1]
    assert asp._L.as_diverse_kernel_us(aspace._h) == 0.0   # (no timed call yet)
    try:
        assert asp._L.as_set_tuning(b"diverse_timing", 1) == 0
        aspace.search_diverse(Q[1], gl, TAU, 10, 0.5)
        assert asp._L.as_diverse_kernel_us(aspace._h) > 0.0
    finally:
        assert asp._L.as_set_tuning(b"diverse_timing", 0) == 0


def test_zz_ambiguous_steps_are_rare():
    """Over every stepwise check of the module (this test runs last): steps whose reference gap is below 100 tol are at most 1 %."""
    print(f"stepwise checks: {TOTAL['steps']} steps, {TOTAL['ambiguous']} ambiguous")
    assert 100 * TOTAL["ambiguous"] <= TOTAL["steps"], TOTAL
