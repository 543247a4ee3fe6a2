"""CPU: the numpy reference of graph eigenpairs (tests/spectral_ref.py) and the inputs of
tests/test_gpu_spectral.py, shown on the numpy oracle's build of the same items with the reference alone.  The vectorised
primitives agree in bits with the SPEC's loops (n = 37, C = 16; the Gram and the column norms also at n = 2 053: three Gram segments
in a tree padded to four, 33 dot segments; and one row and one column of the Gram and the column norms at n = 33 797, the size of
tests/test_gpu_diffusion_scale.py: 34 and 529 segments in trees padded to 64 and 1 024).  On shapes A and B of diffuse_ref.SHAPES
the eigenvalue 1 of S has multiplicity 8 and 19, the gap behind it is >= 0.1 and >= 0.05, -1 is attained and rows without an edge
exist.  The reference driver converges for every (shape, m) of the GPU test within 40 outer iterations (the GPU test allows 60).
Its orthonormality defect max |V V^T - I| over those cases is printed; the largest seen is 2.9e-15, recorded as
spectral_ref.ORTHO_DEFECT = 3e-15, and the GPU test's bound is 100 times that.
Shape C of diffuse_ref.SCALE_SHAPES (2 053 items: three Gram segments) is the scale test's: 352 rows without an edge, a longest
row of 39 entries, the eigenvalue 1 with multiplicity 19 and the next value 0.99877 (a gap of 1.2e-3), -1 attained.  The reference
driver converges there for m = 8, 13, 19 and 48 in 21, 4, 4 and 7 outer iterations (341, 49, 49 and 100 graph passes) with a
defect of at most 2.8e-15, inside the same ORTHO_DEFECT."""
import numpy as np
import pytest

import diffuse_ref as dfr
import diffuse_solve_ref as dsr
import spectral_ref as spr
from oracle import oracle_np
from test_diffuse_api import csr_of, random_graph

_built = {}


def bits(a):
    return dfr.canon(a).tolist()


def fixture(name):
    """(operator, eigenvalues of the dense S descending) of a shape, once per module."""
    if name not in _built:
        X, gp = dfr.shape_items(name)
        idx = oracle_np.build(X, gp)
        op = (np.asarray(idx["indptr"], dtype=np.int64), np.asarray(idx["indices"], dtype=np.int64), -np.asarray(idx["lap"], dtype=np.float64))
        _built[name] = (op, np.linalg.eigvalsh(dsr.dense_operator(*op))[::-1].copy())
    return _built[name]


def test_vectorised_and_loop_forms_agree_in_bits():
    n, C = 37, 16
    p, c, S = dfr.operator(*csr_of(n, random_graph(n - 2, np.random.default_rng(3))))   # the last two rows have no edge
    V, W = spr.hand_block(n, C, 1), spr.hand_block(n, C, 2)
    rows = dsr.RowSums(p, c, S)
    for a, b, g in ((1.0, 0.0, 0.0), (1.7, -0.3, 0.0), (2.1, -0.4, -1.0)):
        assert bits(spr.step(rows, V, a, b, g, W)) == bits(spr.step_loops(p, c, S, V, a, b, g, W))
    assert bits(spr.step(rows, V, 1.7, -0.3)) != bits(spr.step(rows, V, 1.7, -0.3, -1.0, W))
    assert bits(spr.gram(V, W)) == bits(spr.gram_loops(V, W))
    assert bits(spr.gram(V, V)) == bits(spr.gram_loops(V, V))
    T = spr.hand_block(C, C, 3)
    assert bits(spr.rotate(V, T)) == bits(spr.rotate_loops(V, T))
    theta = np.random.default_rng(4).uniform(-1.0, 1.0, C)
    assert bits(spr.colnorm2(V, W, theta)) == bits(spr.colnorm2_loops(V, W, theta))
    for seed in (0, 7, 2 ** 63 - 1):
        blk = spr.start_block(n, C, seed)
        assert bits(blk) == bits(spr.start_block_loops(n, C, seed))
        assert blk.min() >= -0.5 and blk.max() < 0.5 and abs(blk.mean()) < 0.05
    assert bits(spr.start_block(n, C, 0)) != bits(spr.start_block(n, C, 1))


def test_the_trees_of_the_gram_and_of_the_column_norms():
    n, C = 2053, 16
    A, B = spr.hand_block(n, C, 5), spr.hand_block(n, C, 6)
    assert -(-n // spr.GRAM_SEG) == 3 and -(-n // dsr.SEG) == 33
    G = spr.gram(A, B)
    assert bits(G) == bits(spr.gram_loops(A, B))
    assert bits(G) != bits(A.T @ B)   # (the order is under test: the plain product differs)
    theta = np.random.default_rng(7).uniform(-1.0, 1.0, C)
    assert bits(spr.colnorm2(A, B, theta)) == bits(spr.colnorm2_loops(A, B, theta))
    # the size of tests/test_gpu_diffusion_scale.py: 34 Gram segments in a tree padded to 64 and 529 dot segments in one padded to
    # 1 024, so the first level of either adds a real upper half to its first pairs (2 and 17) and +0.0 to the others
    n = 33797
    A, B = spr.hand_block(n, C, 8), spr.hand_block(n, C, 9)
    assert -(-n // spr.GRAM_SEG) == 34 and -(-n // dsr.SEG) == 529
    G = spr.gram(A, B)
    assert bits(G[3:4]) == bits(spr.gram_loops(A[:, 3:4], B))     # one row
    assert bits(G[:, 11:12]) == bits(spr.gram_loops(A, B[:, 11:12]))   # one column
    assert bits(G) != bits(A.T @ B)
    assert bits(spr.colnorm2(A, B, theta)) == bits(spr.colnorm2_loops(A, B, theta))


@pytest.mark.parametrize("name, mult, gap", [("A", 8, 0.1), ("B", 19, 0.05), ("C", 19, 1e-3)])
def test_the_spectrum_of_the_shapes(name, mult, gap):
    op, ev = fixture(name)
    assert int((ev > 1.0 - 1e-9).sum()) == mult and ev[0] <= 1.0 + 1e-12
    print(f"{name}: the eigenvalue 1 has multiplicity {mult}, the next is {ev[mult]:.6f}, the smallest {ev[-1]:.16f}")
    assert 1.0 - ev[mult] >= gap
    assert abs(ev[-1] + 1.0) <= 1e-12               # -1 is attained
    assert (np.diff(op[0]) == 0).sum() >= 1         # rows without an edge
    assert np.diff(op[0]).max() >= 24               # a long row
    n = len(op[0]) - 1
    assert n % 64 != 0 and n >= 64


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_the_reference_driver_converges_on_the_gpu_tests_cases(name):
    driver_converges(name, spr.CASES)


def test_the_reference_driver_converges_on_shape_c_at_a_gap_of_a_thousandth():
    op, ev = fixture("C")
    assert len(op[0]) - 1 == 2053 and -(-2053 // spr.GRAM_SEG) == 3   # more than one Gram partial in every sum of the driver
    driver_converges("C", spr.SCALE_CASES)
    # m = 13 asks for 13 of the 19 copies of the value 1; m >= 19 for all of them and the gap behind
    assert (np.abs(ev[:19] - 1.0) <= 1e-12).all() and ev[19] < 1.0 - 1e-3


def driver_converges(name, cases):
    op, ev = fixture(name)
    worst = 0.0
    for m, C in cases:
        vals, vecs, info = spr.eigs(*op, m, spr.TOL, spr.MAX_ITERS)
        defect = float(np.abs(vecs @ vecs.T - np.eye(m)).max())
        worst = max(worst, defect)
        print(f"{name} m {m} C {C}: {info['iterations']} outer iterations, {info['filter_steps']} steps, |theta - lambda| up to "
              f"{np.abs(vals - ev[:m]).max():.2e}, residual up to {info['residuals'].max():.2e}, orthonormality defect {defect:.2e}")
        assert info["block"] == C and info["converged"] and info["iterations"] <= 40
        assert (info["residuals"] <= spr.TOL).all()
        assert (np.abs(vals - ev[:m]) <= spr.TOL + 1e-12).all()
        assert (np.diff(vals) <= 0.0).all()
        it = info["iterations"]
        assert (info["gram"], info["rotate"]) == (3 * it, 4 * it)
        for j in range(m):   # the sign rule
            assert vecs[j, int(np.argmax(np.abs(vecs[j])))] > 0.0
    assert worst <= spr.ORTHO_DEFECT


def test_a_stop_at_max_iters_leaves_an_orthonormal_iterate():
    op, _ = fixture("A")
    vals, vecs, info = spr.eigs(*op, 8, spr.TOL, 1)
    assert not info["converged"] and info["iterations"] == 1 and info["filter_steps"] == 1
    assert np.abs(vecs @ vecs.T - np.eye(8)).max() <= spr.ORTHO_DEFECT and (np.diff(vals) <= 0.0).all()
    op, _ = fixture("B")
    vals, vecs, info = spr.eigs(*op, 8, spr.TOL, 2, degree=1)
    assert not info["converged"] and info["iterations"] == 2 and info["filter_steps"] == 3


def test_the_filter_plan():
    # a well separated top: the cap on the growth shortens the filter; a top close to the cut: the whole degree
    e, c, d = spr.filter_plan(np.array([1.0, 0.9, 0.0]), 16)
    assert (e, c) == (0.5, -0.5) and d == int(np.floor(np.log(2e6) / np.arccosh(3.0)))
    e, c, d = spr.filter_plan(np.array([1.0, 0.9999, 0.9998]), 16)
    assert c + e == pytest.approx(1.0 - 2e-3) and d == 16     # the floor on the gap, not the smallest Ritz value
    e, c, d = spr.filter_plan(np.array([1.0, 0.5, -1.0]), 16)
    assert e > 0.0 and d == 1                                 # a Ritz value at lo: the interval keeps a width
