"""GPU: fixed-point diffusion search -- ArrowSpace.diffuse_solve / search_diffuse_solve / search_batch_diffuse_solve /
score_diffuse_solve / score_diffuse_solve_batch.  Every expected value comes from tests/diffuse_solve_ref.py on
`gl.to_csr()` and, for the search and score forms, on the pool that the ordinary route returns on the GPU in the same test, so only
the new code is under test.  The shapes, the indices and the helpers are those of tests/test_gpu_diffuse.py (one index per shape
for both modules); every call runs under "diffuse_tile_edges" = 8, so long rows span LDS tiles.
tests/test_diffuse_solve_inputs.py shows the properties of the inputs the checks lean on."""
import ctypes as C

import numpy as np
import pytest

import diffuse_ref as dfr
import diffuse_solve_ref as dsr
from test_gpu_diffuse import Index, _built, batch_pools, bits, index, same_list, tune
from conftest import calibrate_feature_eps, clustered

pytestmark = pytest.mark.gpu

TAU = dfr.TAU
TILE = {b"diffuse_tile_edges": dfr.TILE_EDGES}
_ref = {}
_dense = {}
NAMES = ("calls", "route searches", "column chunks", "iterations launched", "host waits", "seeds uploaded")


def columns(ix):
    return dsr.seed_columns(ix.n, ix.gp["topk"])


def reference(name, alpha, tol):
    """The reference's (F [n, 70], iterations, residual, converged) of the fixture's columns over the device's to_csr(): once."""
    key = (name, alpha, tol)
    if key not in _ref:
        ix = index(name)
        Y = np.stack([dfr.seeds_vector(ix.n, i, v) for i, v in columns(ix)], axis=1)
        _ref[key] = dsr.solve(*ix.op, Y, alpha, tol, 100)
    return _ref[key]


def dense(name):
    if name not in _dense:
        _dense[name] = dsr.dense_operator(*index(name).op)
    return _dense[name]


def same_solve(got, info, want, cols, what=None):
    """The raw form's (f, info) for the fixture's columns `cols` against the reference's tuple: f in bits (the sign of a zero is
    free), the iteration counts, the residual's bits and the converged flags."""
    F, it, res, conv = want
    assert got.shape == (len(cols), F.shape[0]) and got.dtype == np.float64
    assert (dfr.canon(got) == dfr.canon(F[:, cols].T)).all(), what
    assert info["iterations"].tolist() == it[cols].tolist(), what
    assert info["residual"].view(np.uint64).tolist() == np.ascontiguousarray(res[cols]).view(np.uint64).tolist(), what
    assert info["converged"].tolist() == conv[cols].tolist(), what


def counters(ix):
    out = (C.c_int64 * 6)()
    assert ix.asp._L.as_diffuse_solve_counters(ix.aspace._h, out, 6) == 0
    return list(out)


def pool_ref(ix, pool, alpha, tol, max_iters=100):
    y = dfr.seeds_vector(ix.n, [i for i, _ in pool], [v for _, v in pool])
    return dsr.solve(*ix.op, y, alpha, tol, max_iters)


def pool_seeds(pool):
    keep = [(i, v) for i, v in pool if np.isfinite(v)]
    return (np.array([i for i, _ in keep], dtype=np.int64), np.array([v for _, v in keep], dtype=np.float64))


@pytest.mark.parametrize("cols", [1, 16, 64])
@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_raw_form_bits_iterations_and_residual(name, cols):
    ix = index(name)
    aspace, gl = ix.aspace, ix.gl
    seeds = columns(ix)
    # one column per chunk has nothing to freeze: six columns do; the wider chunks take all 70 (64 + 6, or 4 x 16 + 6)
    use = list(range(6 if cols == 1 else dsr.NCOL))
    try:
        for cap in (0, 1):
            tune(ix, {**TILE, b"diffuse_cols": cols, b"diffuse_grid_cap": cap})
            for alpha in dsr.ALPHAS:
                for tol in dsr.TOLS:
                    want = reference(name, alpha, tol)
                    got, info = aspace.diffuse_solve(gl, [seeds[c] for c in use], alpha, tol)
                    same_solve(got, info, want, use, (cols, cap, alpha, tol))
                    if cap == 0 and alpha == 0.85:
                        again, info2 = aspace.diffuse_solve(gl, [seeds[c] for c in use], alpha, tol)   # the same call twice
                        assert (again.view(np.uint64) == got.view(np.uint64)).all()
                        assert all((info2[k] == info[k]).all() for k in info)
    finally:
        tune(ix, {})


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_seventy_columns_equal_seventy_single_calls(name):
    ix = index(name)
    aspace, gl = ix.aspace, ix.gl
    seeds = columns(ix)
    alpha, tol = 0.85, 1e-10
    want = reference(name, alpha, tol)
    assert len(set(want[1].tolist())) >= 3   # (columns freeze while others go on: test_diffuse_solve_inputs.py)
    try:
        tune(ix, TILE)
        c0 = counters(ix)
        got, info = aspace.diffuse_solve(gl, seeds, alpha, tol)
        c1 = counters(ix)
        same_solve(got, info, want, list(range(dsr.NCOL)))
        # a 64-wide chunk and a 16-wide one for the remaining six; a chunk runs as long as its slowest column
        launched = int(want[1][:64].max() + want[1][64:].max())
        assert [a - b for a, b in zip(c1, c0)] == [1, 0, 2, launched, launched + 2, dsr.NCOL * ix.gp["topk"]]
        for c in range(dsr.NCOL):
            one, oi = aspace.diffuse_solve(gl, [seeds[c]], alpha, tol)
            assert (dfr.canon(one[0]) == dfr.canon(got[c])).all(), c
            assert (int(oi["iterations"][0]), bool(oi["converged"][0])) == (int(info["iterations"][c]), bool(info["converged"][c]))
            assert oi["residual"].view(np.uint64)[0] == info["residual"].view(np.uint64)[c]
        c2 = counters(ix)
        assert [a - b for a, b in zip(c2, c1)][:4] == [dsr.NCOL, 0, dsr.NCOL, int(want[1].sum())]
        assert aspace.diffuse_solve_counters() == dict(zip(NAMES, c2))
    finally:
        tune(ix, {})


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_max_iters_alpha_zero_and_a_zero_column(name):
    ix = index(name)
    aspace, gl = ix.aspace, ix.gl
    cols = columns(ix)
    empty = (np.empty(0, dtype=np.int64), np.empty(0))
    seeds = [cols[0], empty, cols[1], cols[2]]
    Y = np.stack([dfr.seeds_vector(ix.n, i, v) for i, v in seeds], axis=1)
    try:
        for setting in ({**TILE}, {**TILE, b"diffuse_cols": 1}):
            tune(ix, setting)
            # max_iters = 3: the third iterate, not converged (the zero column: converged at once)
            want = dsr.solve(*ix.op, Y, 0.85, 1e-10, 3)
            got, info = aspace.diffuse_solve(gl, seeds, 0.85, 1e-10, max_iters=3)
            same_solve(got, info, want, [0, 1, 2, 3])
            assert info["iterations"].tolist() == [3, 0, 3, 3] and info["converged"].tolist() == [False, True, False, False]
            assert info["residual"][1] == 0.0 and (got[1] == 0.0).all() and (info["residual"][[0, 2, 3]] > 1e-10).all()
            assert (dfr.canon(got[0]) != dfr.canon(reference(name, 0.85, 1e-10)[0][:, 0])).any()   # (not the converged answer)
            # alpha = 0: f = y after one iteration
            got, info = aspace.diffuse_solve(gl, seeds, 0.0, 1e-8)
            assert (dfr.canon(got) == dfr.canon(Y.T)).all()
            assert info["iterations"].tolist() == [1, 0, 1, 1] and info["converged"].all() and (info["residual"] == 0.0).all()
    finally:
        tune(ix, {})


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_true_residual_and_distance_to_the_dense_solve(name):
    ix = index(name)
    aspace, gl = ix.aspace, ix.gl
    seeds = columns(ix)
    Y = np.stack([dfr.seeds_vector(ix.n, i, v) for i, v in seeds], axis=1)
    Sd = dense(name)
    try:
        tune(ix, TILE)
        for alpha in dsr.ALPHAS:
            A = np.eye(ix.n) - alpha * Sd
            B = (1.0 - alpha) * Y
            star = np.linalg.solve(A, B)
            nb = np.linalg.norm(B, axis=0)
            for tol in dsr.TOLS:
                got, info = aspace.diffuse_solve(gl, seeds, alpha, tol)
                F = got.T
                true = np.linalg.norm(B - A @ F, axis=0)
                err = np.linalg.norm(F - star, axis=0)
                print(f"{name} alpha {alpha} tol {tol}: true residual / (tol |b|) up to {(true / (tol * nb)).max():.3f}, "
                      f"error / (tol |b| / (1 - alpha)) up to {(err / (tol * nb / (1.0 - alpha))).max():.3f}")
                assert info["converged"].all()
                assert (true <= 2.0 * tol * nb).all()
                assert (err <= 2.0 * tol * nb / (1.0 - alpha)).all()
    finally:
        tune(ix, {})


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_search_and_score_forms(name):
    ix = index(name)
    aspace, gl = ix.aspace, ix.gl
    rng = np.random.default_rng(43)
    Q = ix.queries(rng, 5)
    part = np.sort(rng.choice(ix.n, (2 * ix.n) // 5, replace=False))
    listed = np.concatenate([rng.choice(ix.n, 30), [0, ix.n - 1, 0]]).astype(np.int64)   # (duplicates kept)
    alpha, tol = 0.85, 1e-8
    moved = 0
    try:
        tune(ix, TILE)
        for ids in (None, part):
            sub = None if ids is None else aspace.subset(ids)
            k = ix.topk(ids)
            for q in Q[:3]:
                pool = aspace.search(q, gl, TAU) if sub is None else aspace.search_subset(q, gl, TAU, sub)
                f, it, res, conv = pool_ref(ix, pool, alpha, tol)
                got, info = aspace.search_diffuse_solve(q, gl, TAU, alpha, tol, subset=sub, with_info=True)
                assert len(got) == k
                same_list(got, dfr.rank(f, ids, k))
                assert aspace.search_diffuse_solve(q, gl, TAU, alpha, tol, subset=sub) == got
                moved += [i for i, _ in got] != [i for i, _ in pool[:k]]
                # with_info is the raw form's report on the same seeds
                _, raw = aspace.diffuse_solve(gl, [pool_seeds(pool)], alpha, tol)
                assert info == {"iterations": int(raw["iterations"][0]), "residual": float(raw["residual"][0]), "converged": bool(raw["converged"][0])}
                assert (info["iterations"], info["converged"]) == (it, conv) and info["residual"] == res and conv and it >= 5
            Qb = np.stack(Q)
            pools, st = batch_pools(ix, Qb, TAU, sub)
            assert not any(st)
            got, info = aspace.search_batch_diffuse_solve(Qb, gl, TAU, alpha, tol, subset=sub, with_info=True)
            assert len(got) == 5 and aspace.search_batch_diffuse_solve(Qb, gl, TAU, alpha, tol, subset=sub) == got
            for i, (g, pool) in enumerate(zip(got, pools)):
                f, it, res, conv = pool_ref(ix, pool, alpha, tol)
                same_list(g, dfr.rank(f, ids, k))
                assert (int(info["iterations"][i]), float(info["residual"][i]), bool(info["converged"][i])) == (it, res, conv)
        assert moved >= 2   # (the solve reorders: a no-op implementation cannot pass)
        # the score forms: f at the listed ids, the caller's order
        for q in Q[:3]:
            f, it, res, conv = pool_ref(ix, aspace.search(q, gl, TAU), alpha, tol)
            got, info = aspace.score_diffuse_solve(q, gl, TAU, alpha, listed, tol, with_info=True)
            assert got.shape == listed.shape and bits(got) == bits(f[listed])
            assert info == {"iterations": it, "residual": res, "converged": conv}
        pools, _ = batch_pools(ix, np.stack(Q), TAU, None)
        got = aspace.score_diffuse_solve_batch(np.stack(Q), gl, TAU, alpha, listed, tol)
        assert got.shape == (5, len(listed))
        for g, pool in zip(got, pools):
            assert bits(g) == bits(pool_ref(ix, pool, alpha, tol)[0][listed])
        assert aspace.score_diffuse_solve(Q[0], gl, TAU, alpha, [], tol).shape == (0,)
        assert aspace.search_diffuse_solve(Q[0], gl, TAU, alpha, tol, subset=[]) == []
    finally:
        tune(ix, {})


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_consequence_a_alpha_zero_returns_the_routes_list(name):
    ix = index(name)
    aspace, gl = ix.aspace, ix.gl
    Q = ix.queries(np.random.default_rng(5), 5)
    for q in Q:
        pool = aspace.search(q, gl, TAU)
        assert len(pool) == ix.gp["topk"] and min(v for _, v in pool) > 0.0
        got, info = aspace.search_diffuse_solve(q, gl, TAU, 0.0, with_info=True)
        assert got == pool and info == {"iterations": 1, "residual": 0.0, "converged": True}
    pools, _ = batch_pools(ix, np.stack(Q), TAU, None)
    assert aspace.search_batch_diffuse_solve(np.stack(Q), gl, TAU, 0.0) == pools


def test_zero_lambda():
    ix = index("B")
    asp, aspace, gl = ix.asp, ix.aspace, ix.gl
    near = ix.queries(np.random.default_rng(9), 2)
    far = np.ascontiguousarray(np.full(ix.d, 50.0))   # no item within eps: lambda_q == 0
    alpha, tol = 0.5, 1e-8
    c0 = counters(ix)
    for s in (None, [1, 2, 3]):
        with pytest.raises(asp.PanicException):
            aspace.search_diffuse_solve(far, gl, TAU, alpha, tol, subset=s)
    with pytest.raises(asp.PanicException):
        aspace.score_diffuse_solve(far, gl, TAU, alpha, [1, 2], tol)
    c1 = counters(ix)
    assert c1[2:] == c0[2:]   # no chunk, no iteration, no wait, no seed
    Qb = np.stack([near[0], far, near[1]])
    pools, st = batch_pools(ix, Qb, TAU, None)
    assert [v != 0 for v in st] == [False, True, False]
    got, info = aspace.search_batch_diffuse_solve(Qb, gl, TAU, alpha, tol, with_info=True)
    assert got[1] == []
    assert info["iterations"][1] == 0 and not info["converged"][1] and np.isnan(info["residual"][1])
    refs = {i: pool_ref(ix, pools[i], alpha, tol) for i in (0, 2)}
    for i in (0, 2):
        same_list(got[i], dfr.rank(refs[i][0], None, ix.topk()))
        assert (int(info["iterations"][i]), bool(info["converged"][i])) == (refs[i][1], True)
    sc = aspace.score_diffuse_solve_batch(Qb, gl, TAU, alpha, [5, 6, 7], tol)
    assert np.isnan(sc[1]).all()
    for i in (0, 2):
        assert bits(sc[i]) == bits(refs[i][0][[5, 6, 7]])
    c2 = counters(ix)
    launched = max(refs[0][1], refs[2][1])
    assert [a - b for a, b in zip(c2, c1)][2:5] == [2, 2 * launched, 2 * launched + 2]   # one chunk of two served columns per call


def test_the_recurrence_is_untouched_by_a_solve_between():
    ix = index("B")
    aspace, gl = ix.aspace, ix.gl
    seeds = columns(ix)[:20]
    Y = np.stack([dfr.seeds_vector(ix.n, i, v) for i, v in seeds], axis=1)
    before = aspace.diffuse(gl, seeds, 0.85, 3)
    assert (dfr.canon(before) == dfr.canon(dfr.diffuse(*ix.op, Y, 0.85, 3).T)).all()
    aspace.diffuse_solve(gl, columns(ix), 0.99, 1e-10)
    after = aspace.diffuse(gl, seeds, 0.85, 3)
    assert (after.view(np.uint64) == before.view(np.uint64)).all()
    one = aspace.diffuse(gl, seeds[:1], 0.85, 3)
    aspace.diffuse_solve(gl, seeds[:1], 0.5, 1e-6)
    assert (aspace.diffuse(gl, seeds[:1], 0.85, 3).view(np.uint64) == one.view(np.uint64)).all()


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
    for alpha, tol, mi, word in ((-0.1, 1e-8, 10, "alpha must"), (1.0, 1e-8, 10, "alpha must"), (float("nan"), 1e-8, 10, "alpha must"),
                                 (0.5, 0.0, 10, "tol must"), (0.5, float("inf"), 10, "tol must"), (0.5, float("nan"), 10, "tol must"),
                                 (0.5, 1e-8, 0, "max_iters must"), (0.5, 1e-8, 1025, "max_iters must")):
        assert L.as_search_diffuse_solve(aspace._h, gl._h, q.ctypes.data, d, TAU, alpha, tol, mi, None, idx.ctypes.data, sc.ctypes.data,
                                         C.byref(ln), None, None, None, None) == EINVAL
        assert word in asp._lib.last_error() and ln.value == 0
        assert L.as_search_diffuse_solve_batch(aspace._h, gl._h, Q2.ctypes.data, 2, d, TAU, alpha, tol, mi, None, idx.ctypes.data,
                                               sc.ctypes.data, ln2.ctypes.data, None, None, None, None, None) == EINVAL
        assert L.as_score_diffuse_solve_batch(aspace._h, gl._h, Q2.ctypes.data, 2, d, TAU, alpha, tol, mi, one.ctypes.data, 1,
                                              out.ctypes.data, None, None, None, None, None) == EINVAL
        assert L.as_diffuse_solve_seeds(aspace._h, gl._h, one.ctypes.data, val.ctypes.data, offs.ctypes.data, 1, alpha, tol, mi,
                                        out.ctypes.data, None, None, None) == EINVAL
        for call in (lambda: aspace.search_diffuse_solve(q, gl, TAU, alpha, tol, mi), lambda: aspace.search_batch_diffuse_solve(Q2, gl, TAU, alpha, tol, mi),
                     lambda: aspace.score_diffuse_solve(q, gl, TAU, alpha, [1], tol, mi), lambda: aspace.score_diffuse_solve_batch(Q2, gl, TAU, alpha, [1], tol, mi),
                     lambda: aspace.diffuse_solve(gl, [([3], [1.0])], alpha, tol, mi)):
            with pytest.raises(ValueError):
                call()
    for bad_ids, bad_vals in (([ix.n], [1.0]), ([3], [float("inf")]), ([3, 3], [1.0, 2.0])):
        with pytest.raises(ValueError):
            aspace.diffuse_solve(gl, [(bad_ids, bad_vals)], 0.5)
    assert counters(ix) == c0
    if "feature" not in _built:
        X = clustered(300, 12, nclust=6, seed=18)
        gp = {"eps": calibrate_feature_eps(X, 4), "k": 4, "topk": 8, "p": 2.0, "sigma": None, "metric": "cosine", "kernel": "rational",
              "lambda_mode": "feature"}
        _built["feature"] = Index(X, gp)
    fx = _built["feature"]
    fq = fx.queries(np.random.default_rng(19), 1)[0]
    f0 = counters(fx)
    assert L.as_diffuse_solve_seeds(fx.aspace._h, fx.gl._h, one.ctypes.data, val.ctypes.data, offs.ctypes.data, 1, 0.5, 1e-8, 10,
                                    out.ctypes.data, None, None, None) == EUNSUPPORTED
    for call in (lambda: fx.aspace.search_diffuse_solve(fq, fx.gl, TAU, 0.5), lambda: fx.aspace.search_batch_diffuse_solve(fq[None, :], fx.gl, TAU, 0.5),
                 lambda: fx.aspace.score_diffuse_solve(fq, fx.gl, TAU, 0.5, [1]), lambda: fx.aspace.diffuse_solve(fx.gl, [([3], [1.0])], 0.5)):
        with pytest.raises(ValueError, match="feature-mode"):
            call()
    assert counters(fx) == f0
