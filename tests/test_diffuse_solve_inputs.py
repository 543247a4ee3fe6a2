"""CPU: the inputs of tests/test_gpu_diffuse_solve.py have the properties its checks lean on, shown on the numpy oracle's build of
the same items with the reference alone: for every alpha and tol of the GPU test the fixture's seed columns reach at least three
distinct iteration counts (so columns freeze while others go on) and one of at least 10, the true residual and the distance to
the dense solve stay inside S20's bounds; and S19's properties of the shapes still hold.  The same is shown for shape C of
diffuse_ref.SCALE_SHAPES with the 40 seed columns of tests/test_gpu_diffusion_scale.py."""
import numpy as np
import pytest

import diffuse_ref as dfr
import diffuse_solve_ref as dsr
from oracle import oracle_np

_built = {}


def fixture(name):
    """(n, operator, dense S, seed matrix Y) of a shape, once per module."""
    if name not in _built:
        X, gp = dfr.shape_items(name)
        idx = oracle_np.build(X, gp)
        n = X.shape[0]
        # the oracle keeps the rows as to_csr() gives them less the diagonal; `lap` holds the Laplacian's entries: S = -lap
        op = (np.asarray(idx["indptr"], dtype=np.int64), np.asarray(idx["indices"], dtype=np.int64), -np.asarray(idx["lap"], dtype=np.float64))
        Y = np.stack([dfr.seeds_vector(n, i, v) for i, v in dsr.seed_columns(n, gp["topk"], count=COLUMNS.get(name, dsr.NCOL))], axis=1)
        _built[name] = (n, op, dsr.dense_operator(*op), Y)
    return _built[name]


COLUMNS = {"C": 40}   # the seed columns of tests/test_gpu_diffusion_scale.py's budget test on shape C of diffuse_ref.SCALE_SHAPES


@pytest.mark.parametrize("name", list(dfr.SHAPES) + ["C"])
def test_the_operator_is_symmetric_with_spectrum_in_minus_one_to_one(name):
    n, op, Sd, _ = fixture(name)
    assert (Sd == Sd.T).all()
    ev = np.linalg.eigvalsh(Sd)
    assert ev.min() >= -1.0 - 1e-12 and ev.max() <= 1.0 + 1e-12


@pytest.mark.parametrize("tol", dsr.TOLS)
@pytest.mark.parametrize("alpha", dsr.ALPHAS)
@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_iteration_counts_and_error_bounds_of_the_gpu_fixture(name, alpha, tol):
    counts_and_bounds(name, alpha, tol)


def test_iteration_counts_and_error_bounds_of_the_forty_columns_on_shape_c():
    """What the budget test of tests/test_gpu_diffusion_scale.py runs: 40 columns, alpha 0.85, tol 1e-10 (26 .. 36 iterations)."""
    n, _, _, Y = fixture("C")
    assert Y.shape == (2053, 40)
    it = counts_and_bounds("C", 0.85, 1e-10)
    # three chunks of 16, 16 and 8 columns each hold columns that freeze while others go on
    assert all(len(set(it[s:s + 16].tolist())) >= 2 for s in (0, 16, 32))


def counts_and_bounds(name, alpha, tol):
    n, op, Sd, Y = fixture(name)
    F, it, res, conv = dsr.solve(*op, Y, alpha, tol, 100)
    A = np.eye(n) - alpha * Sd
    B = (1.0 - alpha) * Y
    star = np.linalg.solve(A, B)
    nb = np.linalg.norm(B, axis=0)
    true = np.linalg.norm(B - A @ F, axis=0) / nb
    err = np.linalg.norm(F - star, axis=0) / (nb / (1.0 - alpha))
    print(f"{name} alpha {alpha} tol {tol}: iterations {it.tolist()}, true residual / tol {np.round(true / tol, 3).tolist()}, "
          f"error / (tol |b| / (1 - alpha)) {np.round(err / tol, 3).tolist()}")
    assert conv.all() and (res <= tol).all()
    assert len(set(it.tolist())) >= 3, it
    assert it.max() >= 10
    assert (true <= 2.0 * tol).all()
    assert (err <= 2.0 * tol).all()
    return it


@pytest.mark.parametrize("name", list(dfr.SHAPES) + ["C"])
def test_the_shapes_keep_the_rows_the_kernels_must_survive(name):
    n, op, _, _ = fixture(name)
    deg = np.diff(op[0])
    assert (deg == 0).sum() >= 1                  # a row without an edge
    assert deg.max() >= 3 * dfr.TILE_EDGES        # a row of at least three LDS tiles
    assert n % 64 != 0 and n > 256                # a partial last segment, more than one 256-row group
