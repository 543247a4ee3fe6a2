"""GPU: graph eigenpairs -- ArrowSpace.eigsh and the four device primitives behind it.  The primitives are pinned in
bits against tests/spectral_ref.py through the debug entry `_spectral_op`, which makes exactly the driver's launches.  The driver's
answer depends on the roundings of the host eigensolver and is checked by what an eigenpair must satisfy, against numpy's `eigh`
of the dense S of `gl.to_csr()`.  The shapes, the indices and the helpers are those of tests/test_gpu_diffuse.py (one index per
shape for the three modules).  tests/test_spectral_inputs.py shows the properties of the inputs the checks lean on, and records
the reference's orthonormality defect: the bound here is 100 times spectral_ref.ORTHO_DEFECT."""
import ctypes as C

import numpy as np
import pytest

import diffuse_ref as dfr
import diffuse_solve_ref as dsr
import spectral_ref as spr
from test_gpu_diffuse import Index, _built, index, tune
from conftest import calibrate_eps, calibrate_feature_eps, clustered

pytestmark = pytest.mark.gpu

TOL, MAX_ITERS = spr.TOL, spr.MAX_ITERS
ORTHO = 100.0 * spr.ORTHO_DEFECT
NAMES = ("calls", "outer iterations", "step launches", "gram launches", "rotate launches", "host waits")
_dense = {}
_rows = {}


def dense(name):
    """(dense S, its eigenvalues descending, its eigenvectors as columns in that order) over the device's to_csr(): once."""
    if name not in _dense:
        Sd = dsr.dense_operator(*index(name).op)
        w, V = np.linalg.eigh(Sd)
        _dense[name] = (Sd, w[::-1].copy(), np.ascontiguousarray(V[:, ::-1]))
    return _dense[name]


def rowsums(name):
    if name not in _rows:
        _rows[name] = dsr.RowSums(*index(name).op)
    return _rows[name]


def counters(ix):
    out = (C.c_int64 * 6)()
    assert ix.asp._L.as_graph_eigs_counters(ix.aspace._h, out, 6) == 0
    return list(out)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert (dfr.canon(got) == dfr.canon(want)).all(), what


@pytest.mark.parametrize("cols", [16, 64])
@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_step_bits(name, cols):
    ix = index(name)
    rows = rowsums(name)
    V, W = spr.hand_block(ix.n, cols, 11), spr.hand_block(ix.n, cols, 12)
    assert (ix.deg == 0).any() and ix.deg.max() >= 24 and ix.n % 64 != 0   # rows without an edge, long rows, a partial last group
    try:
        for cap in (0, 1):
            tune(ix, {b"diffuse_grid_cap": cap})
            for a, b, g in ((1.0, 0.0, 0.0), (1.7, -0.3, 0.0), (2.1, -0.4, -1.0)):
                want = spr.step(rows, V, a, b, g, W)
                same_bits(ix.aspace._spectral_op(ix.gl, "step", V, W if g else None, coef=(a, b, g)), want, (cap, a, b, g))
                if g:
                    same_bits(ix.aspace._spectral_op(ix.gl, "step", V, W, coef=(a, b, g), alias=True), want, (cap, a, b, g, "alias"))
            # W is not read with g == 0: a block of NaN changes nothing
            same_bits(ix.aspace._spectral_op(ix.gl, "step", V, np.full_like(W, np.nan), coef=(1.7, -0.3, 0.0)),
                      spr.step(rows, V, 1.7, -0.3), (cap, "g == 0"))
    finally:
        tune(ix, {})


@pytest.mark.parametrize("cols", [16, 64])
@pytest.mark.parametrize("n", [257, 2053])
def test_gram_rotate_and_colnorm2_bits(n, cols):
    ix = index("A")
    A, B = spr.hand_block(n, cols, 21), spr.hand_block(n, cols, 22)
    T = spr.hand_block(cols, cols, 23)
    theta = np.random.default_rng(24).uniform(-1.0, 1.0, cols) * 10.0 ** np.random.default_rng(25).uniform(-3.0, 3.0, cols)
    want = {"gram": spr.gram(A, B), "gram2": spr.gram(A, A), "rotate": spr.rotate(A, T), "colnorm2": spr.colnorm2(A, B, theta)}
    assert (dfr.canon(want["gram"]) != dfr.canon(A.T @ B)).any()   # (a changed order changes bits)
    try:
        for cap in (0, 1):
            tune(ix, {b"diffuse_grid_cap": cap})
            same_bits(ix.aspace._spectral_op(ix.gl, "gram", A, B), want["gram"], (cap, "gram"))
            same_bits(ix.aspace._spectral_op(ix.gl, "gram", A), want["gram2"], (cap, "gram of a block with itself"))
            same_bits(ix.aspace._spectral_op(ix.gl, "rotate", A, T=T), want["rotate"], (cap, "rotate"))
            same_bits(ix.aspace._spectral_op(ix.gl, "colnorm2", A, B, T=theta), want["colnorm2"], (cap, "colnorm2"))
    finally:
        tune(ix, {})


@pytest.mark.parametrize("m, cols", spr.CASES)
@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_solver(name, m, cols):
    solver_checks(name, m, cols)


def solver_checks(name, m, cols):
    """What an answer of eigsh(m) on a shape must satisfy -> (values, vectors, info, the dense eigenvalues): also the body of
    tests/test_gpu_diffusion_scale.py's solver test."""
    ix = index(name)
    Sd, lam, vec = dense(name)
    c0 = counters(ix)
    values, vectors, info = ix.aspace.eigsh(ix.gl, m, TOL, MAX_ITERS, with_info=True)
    c1 = counters(ix)
    assert values.shape == (m,) and vectors.shape == (m, ix.n) and values.dtype == vectors.dtype == np.float64
    assert info["block"] == cols and info["converged"] and 1 <= info["iterations"] <= MAX_ITERS
    assert info["residuals"].shape == (m,) and (info["residuals"] <= TOL).all()
    assert (np.diff(values) <= 0.0).all()
    # a symmetric matrix has an eigenvalue within |r| of theta; position by position: none was missed
    err = np.abs(values - lam[:m])
    true = np.linalg.norm(Sd @ vectors.T - vectors.T * values[None, :], axis=0)
    defect = np.abs(vectors @ vectors.T - np.eye(m)).max()
    print(f"{name} m {m} C {cols}: {info['iterations']} outer iterations, {info['filter_steps']} steps, |theta - lambda| up to {err.max():.2e}, "
          f"residual up to {info['residuals'].max():.2e} (host: {true.max():.2e}), orthonormality defect {defect:.2e}")
    assert (err <= TOL + 1e-12).all()
    assert (true <= 2.0 * TOL).all()
    assert defect <= ORTHO
    gap = lam[m - 1] - lam[m]
    if (name, m) in (("A", 8), ("B", 19)):
        assert gap >= 0.05
        P = vectors.T @ vectors - vec[:, :m] @ vec[:, :m].T
        dk = np.linalg.norm(P, 2)
        print(f"   gap {gap:.4f}: |P_got - P_dense| {dk:.2e} against {2.0 * np.sqrt(m) * TOL / gap:.2e}")
        assert dk <= 2.0 * np.sqrt(m) * TOL / gap
    for j in range(m):   # the sign rule
        assert vectors[j, int(np.argmax(np.abs(vectors[j])))] > 0.0
    # info and the counters agree: per outer iteration one Gram and two rotates of Rayleigh-Ritz; two Grams and two rotates at the
    # start and behind each filter; the host waits once per Gram, once per residual and once for the answer
    it = info["iterations"]
    assert [a - b for a, b in zip(c1, c0)] == [1, it, info["filter_steps"], 3 * it, 4 * it, 4 * it + 1]
    assert it <= info["filter_steps"] <= it + 16 * (it - 1)
    assert ix.aspace.eigsh_counters() == dict(zip(NAMES, c1))
    two = ix.aspace.eigsh(ix.gl, m, TOL, MAX_ITERS)
    assert len(two) == 2 and (two[0].view(np.uint64) == values.view(np.uint64)).all()
    return values, vectors, info, lam


@pytest.mark.parametrize("m", [8, 19])
@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_determinism_grid_and_seed(name, m):
    ix = index(name)
    same = lambda a, b: (a.view(np.uint64) == b.view(np.uint64)).all()   # noqa: E731
    try:
        v0, x0, i0 = ix.aspace.eigsh(ix.gl, m, TOL, MAX_ITERS, with_info=True)
        v1, x1, i1 = ix.aspace.eigsh(ix.gl, m, TOL, MAX_ITERS, with_info=True)
        assert same(v0, v1) and same(x0, x1) and same(i0["residuals"], i1["residuals"])
        assert {k: v for k, v in i0.items() if k != "residuals"} == {k: v for k, v in i1.items() if k != "residuals"}
        tune(ix, {b"diffuse_grid_cap": 1})
        v2, x2, i2 = ix.aspace.eigsh(ix.gl, m, TOL, MAX_ITERS, with_info=True)
        assert same(v0, v2) and same(x0, x2) and same(i0["residuals"], i2["residuals"]) and i0["iterations"] == i2["iterations"]
        tune(ix, {})
        v3, x3, i3 = ix.aspace.eigsh(ix.gl, m, TOL, MAX_ITERS, seed=7, with_info=True)
        assert i3["converged"] and not same(x0, x3)
        assert (np.abs(v3 - v0) <= 2.0 * TOL).all()
    finally:
        tune(ix, {})


def test_a_stop_at_max_iters_serves_the_iterate():
    ix = index("A")
    values, vectors, info = ix.aspace.eigsh(ix.gl, 8, TOL, 1, with_info=True)
    assert not info["converged"] and info["iterations"] == 1 and info["filter_steps"] == 1
    assert np.abs(vectors @ vectors.T - np.eye(8)).max() <= ORTHO and (np.diff(values) <= 0.0).all()
    assert (info["residuals"] > TOL).any()
    ix = index("B")
    ref = spr.eigs(*ix.op, 8, TOL, 2, degree=1)[2]   # the CPU reference first
    assert not ref["converged"] and ref["iterations"] == 2
    values, vectors, info = ix.aspace.eigsh(ix.gl, 8, TOL, 2, degree=1, with_info=True)
    assert not info["converged"] and info["iterations"] == 2 and info["filter_steps"] == 3
    assert np.abs(vectors @ vectors.T - np.eye(8)).max() <= ORTHO


def test_the_solve_and_the_eigenpairs_share_buffers_and_leave_each_other_alone():
    ix = index("B")
    aspace, gl = ix.aspace, ix.gl
    seeds = dsr.seed_columns(ix.n, ix.gp["topk"])[:20]
    Y = np.stack([dfr.seeds_vector(ix.n, i, v) for i, v in seeds], axis=1)
    want = dsr.solve(*ix.op, Y, 0.85, 1e-10, 100)
    first = aspace.eigsh(gl, 19, TOL, MAX_ITERS)
    got, info = aspace.diffuse_solve(gl, seeds, 0.85, 1e-10)
    assert (dfr.canon(got) == dfr.canon(want[0].T)).all() and info["iterations"].tolist() == want[1].tolist()
    again = aspace.eigsh(gl, 19, TOL, MAX_ITERS)
    assert (again[0].view(np.uint64) == first[0].view(np.uint64)).all() and (again[1].view(np.uint64) == first[1].view(np.uint64)).all()
    step = aspace.diffuse(gl, seeds, 0.85, 3)
    assert (dfr.canon(step) == dfr.canon(dfr.diffuse(*ix.op, Y, 0.85, 3).T)).all()


def test_refusals_launch_nothing():
    ix = index("A")
    asp, aspace, gl = ix.asp, ix.aspace, ix.gl
    L, EINVAL, EUNSUPPORTED = asp._L, asp._lib.AS_EINVAL, asp._lib.AS_EUNSUPPORTED
    val, vec, res = np.zeros(48), np.zeros((48, ix.n)), np.zeros(48)
    info = np.zeros(4, dtype=np.int64)
    c0 = counters(ix)

    def raw(h, g, m, tol, mi, deg, seed):
        return L.as_graph_eigs(h, g, m, tol, mi, deg, seed, val.ctypes.data, vec.ctypes.data, res.ctypes.data, info.ctypes.data)

    for m, tol, mi, deg, seed, word in ((0, 1e-8, 10, 16, 0, "m must"), (49, 1e-8, 10, 16, 0, "m must"), (8, 0.0, 10, 16, 0, "tol must"),
                                        (8, 1.0, 10, 16, 0, "tol must"), (8, float("nan"), 10, 16, 0, "tol must"),
                                        (8, float("inf"), 10, 16, 0, "tol must"), (8, 1e-8, 0, 16, 0, "max_iters must"),
                                        (8, 1e-8, 10001, 16, 0, "max_iters must"), (8, 1e-8, 10, 0, 0, "degree must"),
                                        (8, 1e-8, 10, 65, 0, "degree must"), (8, 1e-8, 10, 16, -1, "seed must")):
        assert raw(aspace._h, gl._h, m, tol, mi, deg, seed) == EINVAL
        assert word in asp._lib.last_error()
    assert L.as_graph_eigs(aspace._h, gl._h, 8, 1e-8, 10, 16, 0, None, vec.ctypes.data, res.ctypes.data, info.ctypes.data) == EINVAL
    # four blocks beyond the budget: 257 x 64 doubles x 4 is 514 KiB, within 1 MiB; 257 x 16 fits
    other = index("B")
    try:
        assert L.as_set_tuning(b"spectral_mib", 1) == 0
        with pytest.raises(ValueError, match="spectral_mib"):
            other.aspace.eigsh(other.gl, 13)          # 1000 x 64 x 8 x 4 = 1.95 MiB
        assert aspace.eigsh(gl, 13, TOL, MAX_ITERS, with_info=True)[2]["converged"]
    finally:
        assert L.as_set_tuning(b"spectral_mib", 0) == 0
    c1 = counters(ix)
    assert c1[0] == c0[0] + 1
    # the graph of another space
    with pytest.raises(ValueError):
        aspace.eigsh(other.gl, 8)
    # fewer rows than the block's columns
    if "tiny" not in _built:
        X = clustered(40, 8, nclust=2, seed=5)
        _built["tiny"] = Index(X, {"eps": calibrate_eps(X, 4), "k": 4, "topk": 4, "p": 2.0, "sigma": None})
    tiny = _built["tiny"]
    with pytest.raises(ValueError, match="fewer than the 64 columns"):
        tiny.aspace.eigsh(tiny.gl, 13)
    t0 = counters(tiny)
    assert tiny.aspace.eigsh(tiny.gl, 2, 1e-6, MAX_ITERS)[1].shape == (2, 40)   # (40 rows carry a block of 16)
    assert counters(tiny)[0] == t0[0] + 1
    if "feature" not in _built:
        X = clustered(300, 12, nclust=6, seed=18)
        gp = {"eps": calibrate_feature_eps(X, 4), "k": 4, "topk": 8, "p": 2.0, "sigma": None, "metric": "cosine", "kernel": "rational",
              "lambda_mode": "feature"}
        _built["feature"] = Index(X, gp)
    fx = _built["feature"]
    f0 = counters(fx)
    assert raw(fx.aspace._h, fx.gl._h, 8, 1e-8, 10, 16, 0) == EUNSUPPORTED
    with pytest.raises(ValueError, match="feature-mode"):
        fx.aspace.eigsh(fx.gl, 8)
    with pytest.raises(ValueError, match="feature-mode"):
        fx.aspace._spectral_op(fx.gl, "gram", np.zeros((64, 16)))
    assert counters(fx) == f0
    assert counters(ix) == c1
