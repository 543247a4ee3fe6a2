"""GPU: graph-diffusion search -- ArrowSpace.diffuse / search_diffuse / search_batch_diffuse / score_diffuse / score_diffuse_batch
(DESIGN.md S19).  Every expected value comes from tests/diffuse_ref.py on `gl.to_csr()` and, for the search and score forms, on
the pool that the ordinary route (`search`, `search_subset`, `search_batch`, `search_batch_subset`) returns on the GPU in the same
test, so only the new code is under test.  tests/test_diffuse_inputs.py shows the properties of the inputs the checks lean on."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

import diffuse_ref as dfr
from conftest import calibrate_feature_eps, clustered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TAU = dfr.TAU
_built = {}
TUNINGS = (b"diffuse_tile_edges", b"diffuse_cols", b"diffuse_grid_cap")
SETTINGS = ({}, {b"diffuse_tile_edges": dfr.TILE_EDGES}, {b"diffuse_cols": 16}, {b"diffuse_grid_cap": 2}, {b"diffuse_cols": 1},
            {b"diffuse_tile_edges": dfr.TILE_EDGES, b"diffuse_cols": 16, b"diffuse_grid_cap": 2})


class Index:
    """One index with what the checks need: the items, the operator S from to_csr() and its degrees."""

    def __init__(self, X, gp):
        import pyarrowspace_amd as asp
        self.asp, self.X, self.gp = asp, X, gp
        self.aspace, self.gl = asp.ArrowSpaceBuilder.build(gp, X)
        self.n, self.d = X.shape
        if self.gl.lambda_mode != "feature":
            self.op = dfr.operator(*self.gl.to_csr())
            self.deg = np.diff(self.op[0])

    def queries(self, rng, count):
        return dfr.queries_of(self.X, rng, count, lambda q: self.aspace.query_lambda(q, self.gl) != 0.0)

    def ref(self, pool, alpha, steps):
        """f of S19 for a pool [(index, score)]."""
        y = dfr.seeds_vector(self.n, [i for i, _ in pool], [v for _, v in pool])
        return dfr.diffuse(*self.op, y, alpha, steps)

    def topk(self, sub=None):
        return min(self.gp["topk"], self.n, self.n if sub is None else len(sub))


def index(name):
    """One index per shape for the whole module."""
    if name not in _built:
        _built[name] = Index(*dfr.shape_items(name))
    return _built[name]


def tune(ix, setting):
    for key in TUNINGS:
        assert ix.asp._L.as_set_tuning(key, setting.get(key, 0)) == 0


def counters(ix):
    out = (C.c_int64 * 5)()
    assert ix.asp._L.as_diffuse_counters(ix.aspace._h, out, 5) == 0
    return list(out)


def bits(a):
    return dfr.canon(a).tolist()


def same_list(got, want):
    """A returned list [(index, f)] against rank()'s: the indices and the bits of f (the sign of a zero is free)."""
    assert [i for i, _ in got] == [i for i, _ in want]
    assert bits([v for _, v in got]) == bits([v for _, v in want])


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


def raw_seeds(ix, nb, rng):
    """nb seed lists: the first holds a node without an edge, the longest row, one of its neighbours, negative values and
    -0.0; the second is empty; the others are random."""
    lone, hub = int(np.flatnonzero(ix.deg == 0)[0]), int(ix.deg.argmax())
    near = int(ix.op[1][ix.op[0][hub]])
    rest = [int(i) for i in rng.choice(ix.n, 4, replace=False) if int(i) not in (lone, hub, near)]
    seeds = [([lone, hub, near] + rest, [0.75, -1.25, 0.5] + [-0.0, 0.3, -2.0, 1e-3][:len(rest)])]
    for b in range(1, nb):
        m = 0 if b == 1 else int(rng.integers(1, ix.gp["topk"] + 1))
        seeds.append((rng.choice(ix.n, m, replace=False).astype(np.int64), rng.standard_normal(m)))
    return seeds


@pytest.mark.parametrize("nb", [1, 3, 17, 65])
@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_raw_form_bits_under_every_setting(name, nb):
    ix = index(name)
    aspace, gl = ix.aspace, ix.gl
    seeds = raw_seeds(ix, nb, np.random.default_rng(100 + nb))
    Y = np.stack([dfr.seeds_vector(ix.n, i, v) for i, v in seeds], axis=1)
    try:
        for steps in (0, 1, 2, 7):
            for alpha in (0.0, 0.5, 0.99):
                want = dfr.diffuse(*ix.op, Y, alpha, steps).T
                for setting in SETTINGS:
                    tune(ix, setting)
                    got = aspace.diffuse(gl, seeds, alpha, steps)
                    assert got.shape == (nb, ix.n) and got.dtype == np.float64
                    assert (dfr.canon(got) == dfr.canon(want)).all(), (steps, alpha, setting)
                    if not setting:
                        assert (dfr.canon(aspace.diffuse(gl, seeds, alpha, steps)) == dfr.canon(got)).all()   # the same call twice
    finally:
        tune(ix, {})
    # the diffusion moved something: the hub's neighbours rose from 0, the node without an edge received nothing
    f = aspace.diffuse(gl, seeds[:1], 0.5, 2)[0]
    hub, lone = int(ix.deg.argmax()), int(np.flatnonzero(ix.deg == 0)[0])
    nbrs = ix.op[1][ix.op[0][hub]:ix.op[0][hub + 1]]
    assert 2 * np.count_nonzero(f[nbrs]) > len(nbrs) and f[lone] == 0.5 * 0.75


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_search_and_score_forms(name):
    ix = index(name)
    aspace, gl = ix.aspace, ix.gl
    rng = np.random.default_rng(41)
    Q = ix.queries(rng, 5)
    part = np.sort(rng.choice(ix.n, (2 * ix.n) // 5, replace=False))
    few = np.sort(rng.choice(ix.n, ix.gp["topk"] - 3, replace=False))
    listed = np.concatenate([rng.choice(ix.n, 30), [0, ix.n - 1, 0]]).astype(np.int64)   # (duplicates kept)
    alpha, steps = 0.85, 5
    moved = 0
    for ids in (None, part, few):
        sub = None if ids is None else aspace.subset(ids)
        k = ix.topk(ids)
        # the single form on the pool of the single route
        for q in Q[:3]:
            pool = aspace.search(q, gl, TAU) if sub is None else aspace.search_subset(q, gl, TAU, sub)
            f = ix.ref(pool, alpha, steps)
            got = aspace.search_diffuse(q, gl, TAU, alpha, steps, subset=sub)
            assert len(got) == k
            same_list(got, dfr.rank(f, ids, k))
            moved += [i for i, _ in got] != [i for i, _ in pool[:k]]
            if ids is not None:
                assert aspace.search_diffuse(q, gl, TAU, alpha, steps, subset=ids) == got   # an ad-hoc list is the same subset
        # the batched form on the pools of the batched route
        Qb = np.stack(Q)
        pools, st = batch_pools(ix, Qb, TAU, sub)
        assert not any(st)
        got = aspace.search_batch_diffuse(Qb, gl, TAU, alpha, steps, subset=sub)
        assert len(got) == 5
        for g, pool in zip(got, pools):
            same_list(g, dfr.rank(ix.ref(pool, alpha, steps), ids, k))
    assert moved >= 3   # (the diffusion reorders: a no-op implementation cannot pass)
    # the score forms: f at the listed ids, the caller's order
    for q in Q[:3]:
        f = ix.ref(aspace.search(q, gl, TAU), alpha, steps)
        got = aspace.score_diffuse(q, gl, TAU, alpha, steps, listed)
        assert got.shape == listed.shape and bits(got) == bits(f[listed])
    pools, _ = batch_pools(ix, np.stack(Q), TAU, None)
    got = aspace.score_diffuse_batch(np.stack(Q), gl, TAU, alpha, steps, listed)
    assert got.shape == (5, len(listed))
    for g, pool in zip(got, pools):
        assert bits(g) == bits(ix.ref(pool, alpha, steps)[listed])
    assert aspace.score_diffuse(Q[0], gl, TAU, alpha, steps, []).shape == (0,)
    assert aspace.search_diffuse(Q[0], gl, TAU, alpha, steps, subset=[]) == []


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_consequences_a_and_b(name):
    ix = index(name)
    aspace, gl = ix.aspace, ix.gl
    Q = ix.queries(np.random.default_rng(5), 5)
    # (a) steps = 0 or alpha = 0: f = y; the pool is full and every score > 0, so the list is the route's list bit for bit
    for q in Q:
        pool = aspace.search(q, gl, TAU)
        assert len(pool) == ix.gp["topk"] and min(v for _, v in pool) > 0.0
        assert aspace.search_diffuse(q, gl, TAU, 0.85, 0) == pool
        assert aspace.search_diffuse(q, gl, TAU, 0.0, 7) == pool
    pools, _ = batch_pools(ix, np.stack(Q), TAU, None)
    assert aspace.search_batch_diffuse(np.stack(Q), gl, TAU, 0.85, 0) == pools
    assert aspace.search_batch_diffuse(np.stack(Q), gl, TAU, 0.0, 3) == pools
    # (b) column b of a B = 5 call equals the B = 1 call on the same seeds, in bits
    seeds = raw_seeds(ix, 5, np.random.default_rng(77))
    whole = aspace.diffuse(gl, seeds, 0.7, 6)
    for b in range(5):
        assert (dfr.canon(aspace.diffuse(gl, seeds[b:b + 1], 0.7, 6)[0]) == dfr.canon(whole[b])).all()
    other = [seeds[0]] + raw_seeds(ix, 5, np.random.default_rng(78))[1:]
    assert (dfr.canon(aspace.diffuse(gl, other, 0.7, 6)[0]) == dfr.canon(whole[0])).all()


def test_zero_lambda():
    ix = index("B")
    asp, aspace, gl = ix.asp, ix.aspace, ix.gl
    near = ix.queries(np.random.default_rng(9), 2)
    far = np.ascontiguousarray(np.full(ix.d, 50.0))   # no item within eps: lambda_q == 0
    with pytest.raises(asp.PanicException):
        aspace.search(far, gl, TAU)
    c0 = counters(ix)
    for s in (None, [1, 2, 3]):
        with pytest.raises(asp.PanicException):
            aspace.search_diffuse(far, gl, TAU, 0.5, 3, subset=s)
    with pytest.raises(asp.PanicException):
        aspace.score_diffuse(far, gl, TAU, 0.5, 3, [1, 2])
    c1 = counters(ix)
    assert c1[3] == c0[3] and c1[2] == c0[2]
    assert aspace.diffuse_counters()["step launches"] == c0[3]
    Qb = np.stack([near[0], far, near[1]])
    pools, st = batch_pools(ix, Qb, TAU, None)
    assert [v != 0 for v in st] == [False, True, False]
    got = aspace.search_batch_diffuse(Qb, gl, TAU, 0.5, 3)
    assert got[1] == []
    for i in (0, 2):
        same_list(got[i], dfr.rank(ix.ref(pools[i], 0.5, 3), None, ix.topk()))
    sc = aspace.score_diffuse_batch(Qb, gl, TAU, 0.5, 3, [5, 6, 7])
    assert np.isnan(sc[1]).all()
    for i in (0, 2):
        assert bits(sc[i]) == bits(ix.ref(pools[i], 0.5, 3)[[5, 6, 7]])
    c2 = counters(ix)
    assert c2[3] - c1[3] == 6 and c2[2] - c1[2] == 2   # one chunk of two served columns per call, three steps each


def test_refusals_launch_nothing():
    ix = index("A")
    asp, aspace, gl, d = ix.asp, ix.aspace, ix.gl, ix.d
    L, EINVAL, EUNSUPPORTED = asp._L, asp._lib.AS_EINVAL, asp._lib.AS_EUNSUPPORTED
    q = ix.queries(np.random.default_rng(13), 1)[0]
    Q2 = np.stack([q, q * 1.01])
    idx = np.full(64, -1, dtype=np.int64)
    sc = np.zeros(64)
    ln = C.c_int64(-1)
    ln2 = np.zeros(2, dtype=np.int64)
    out = np.zeros(2 * ix.n)
    offs = np.array([0, 1], dtype=np.int64)
    one = np.array([3], dtype=np.int64)
    val = np.array([1.0])
    c0 = counters(ix)
    # the C ABI refuses alpha and steps itself
    for alpha, steps in ((-0.1, 3), (1.0, 3), (float("nan"), 3), (0.5, -1), (0.5, 65)):
        assert L.as_search_diffuse(aspace._h, gl._h, q.ctypes.data, d, TAU, alpha, steps, None, idx.ctypes.data, sc.ctypes.data,
                                   C.byref(ln), None) == EINVAL
        assert ("alpha must" if steps == 3 else "steps must") in asp._lib.last_error() and ln.value == 0
        assert L.as_search_diffuse_batch(aspace._h, gl._h, Q2.ctypes.data, 2, d, TAU, alpha, steps, None, idx.ctypes.data, sc.ctypes.data,
                                         ln2.ctypes.data, None, None) == EINVAL
        assert L.as_score_diffuse_batch(aspace._h, gl._h, Q2.ctypes.data, 2, d, TAU, alpha, steps, one.ctypes.data, 1, out.ctypes.data,
                                        None, None) == EINVAL
        assert L.as_diffuse_seeds(aspace._h, gl._h, one.ctypes.data, val.ctypes.data, offs.ctypes.data, 1, alpha, steps,
                                  out.ctypes.data) == EINVAL
        for call in (lambda: aspace.search_diffuse(q, gl, TAU, alpha, steps), lambda: aspace.search_batch_diffuse(Q2, gl, TAU, alpha, steps),
                     lambda: aspace.score_diffuse(q, gl, TAU, alpha, steps, [1]), lambda: aspace.score_diffuse_batch(Q2, gl, TAU, alpha, steps, [1]),
                     lambda: aspace.diffuse(gl, [([3], [1.0])], alpha, steps)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        aspace.search_diffuse(q, gl, TAU, 0.5, 2.0)
    # ids and seeds
    for bad_ids, bad_vals in (([ix.n], [1.0]), ([-1], [1.0]), ([3], [float("inf")]), ([3, 3], [1.0, 2.0])):
        bi, bv = np.array(bad_ids, dtype=np.int64), np.array(bad_vals)
        bo = np.array([0, len(bad_ids)], dtype=np.int64)
        assert L.as_diffuse_seeds(aspace._h, gl._h, bi.ctypes.data, bv.ctypes.data, bo.ctypes.data, 1, 0.5, 3, out.ctypes.data) == EINVAL
        with pytest.raises(ValueError):
            aspace.diffuse(gl, [(bad_ids, bad_vals)], 0.5, 3)
    with pytest.raises(TypeError):
        aspace.diffuse(gl, [([3.0], [1.0])], 0.5, 3)
    with pytest.raises(ValueError, match="outside"):
        aspace.score_diffuse(q, gl, TAU, 0.5, 3, [ix.n])
    with pytest.raises(ValueError, match="query length"):
        aspace.search_diffuse(np.ascontiguousarray(q[:10]), gl, TAU, 0.5, 3)
    with pytest.raises(ValueError, match="tau"):
        aspace.search_batch_diffuse(Q2, gl, float("inf"), 0.5, 3)
    # a subset of another space; a feature-mode index
    other = index("B")
    with pytest.raises(ValueError, match="another space"):
        aspace.search_diffuse(q, gl, TAU, 0.5, 3, subset=other.aspace.subset([1, 2, 3]))
    assert counters(ix) == c0
    if "feature" not in _built:
        X = clustered(300, 12, nclust=6, seed=18)
        gp = {"eps": calibrate_feature_eps(X, 4), "k": 4, "topk": 8, "p": 2.0, "sigma": None, "metric": "cosine", "kernel": "rational",
              "lambda_mode": "feature"}
        _built["feature"] = Index(X, gp)
    fx = _built["feature"]
    assert fx.gl.lambda_mode == "feature"
    fq = fx.queries(np.random.default_rng(19), 1)[0]
    f0 = counters(fx)
    assert L.as_search_diffuse(fx.aspace._h, fx.gl._h, fq.ctypes.data, fx.d, TAU, 0.5, 3, None, idx.ctypes.data, sc.ctypes.data,
                               C.byref(ln), None) == EUNSUPPORTED
    assert L.as_diffuse_seeds(fx.aspace._h, fx.gl._h, one.ctypes.data, val.ctypes.data, offs.ctypes.data, 1, 0.5, 3,
                              out.ctypes.data) == EUNSUPPORTED
    for call in (lambda: fx.aspace.search_diffuse(fq, fx.gl, TAU, 0.5, 3), lambda: fx.aspace.search_batch_diffuse(fq[None, :], fx.gl, TAU, 0.5, 3),
                 lambda: fx.aspace.score_diffuse(fq, fx.gl, TAU, 0.5, 3, [1]), lambda: fx.aspace.diffuse(fx.gl, [([3], [1.0])], 0.5, 3)):
        with pytest.raises(ValueError, match="feature-mode"):
            call()
    assert counters(fx) == f0


def test_counters_of_hand_counted_calls():
    ix = index("B")
    asp, aspace, gl = ix.asp, ix.aspace, ix.gl
    Q = ix.queries(np.random.default_rng(37), 20)
    topk = ix.gp["topk"]
    c0 = counters(ix)
    aspace.search_diffuse(Q[0], gl, TAU, 0.5, 4)
    c1 = counters(ix)
    assert [a - b for a, b in zip(c1, c0)] == [1, 1, 1, 4, topk]
    aspace.search_batch_diffuse(np.stack(Q), gl, TAU, 0.5, 3)   # 20 queries: a chunk of 16 columns and one of 4
    c2 = counters(ix)
    assert [a - b for a, b in zip(c2, c1)] == [1, 1, 2, 6, 20 * topk]
    aspace.diffuse(gl, [([1, 2], [1.0, 2.0])], 0.5, 0)           # no search, no step
    c3 = counters(ix)
    assert [a - b for a, b in zip(c3, c2)] == [1, 0, 1, 0, 2]
    assert aspace.diffuse_counters() == dict(zip(("calls", "route searches", "column chunks", "step launches", "seeds uploaded"), c3))
    try:
        assert asp._L.as_set_tuning(b"diffuse_timing", 1) == 0
        aspace.search_diffuse(Q[1], gl, TAU, 0.5, 4)
        assert asp._L.as_diffuse_kernel_us(aspace._h) > 0.0
    finally:
        assert asp._L.as_set_tuning(b"diffuse_timing", 0) == 0


def test_two_host_threads_get_the_serial_answers():
    ix = index("B")
    aspace, gl = ix.aspace, ix.gl
    Q = ix.queries(np.random.default_rng(31), 8)
    part = aspace.subset(np.arange(0, ix.n, 3))
    serial = [aspace.search_diffuse(q, gl, TAU, 0.85, 5) for q in Q]
    serial_sub = [aspace.search_diffuse(q, gl, TAU, 0.85, 5, subset=part) for q in Q]
    batch = aspace.search_batch_diffuse(np.stack(Q), gl, TAU, 0.85, 5)
    errors = []

    def run(flip):
        try:
            for q, w, ws in zip(Q, serial, serial_sub):
                if flip:
                    assert aspace.search_diffuse(q, gl, TAU, 0.85, 5, subset=part) == ws
                assert aspace.search_diffuse(q, gl, TAU, 0.85, 5) == w
                if not flip:
                    assert aspace.search_diffuse(q, gl, TAU, 0.85, 5, subset=part) == ws
            assert aspace.search_batch_diffuse(np.stack(Q), gl, TAU, 0.85, 5) == batch
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=run, args=(t == 1,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]
