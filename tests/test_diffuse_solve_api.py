"""CPU: the numpy reference of fixed-point diffusion search (tests/diffuse_solve_ref.py) -- its dot against a
hand-written loop, the vectorised solve against the SPEC's loops on hand-built graphs, its limits and its column independence --
and the Python validators of the solve forms, which run before a handle is touched."""
import numpy as np
import pytest

import diffuse_ref as dfr
import diffuse_solve_ref as dsr
from test_diffuse_api import csr_of, random_graph


def bits(a):
    return dfr.canon(a).tolist()


def hand_dot(u, v):
    """S20's dot, written out: segment sums in row order, padded with +0.0 to a power of two, halved."""
    n = len(u)
    ns = (n + 63) // 64
    sig = []
    for s in range(ns):
        acc = 0.0
        for i in range(64 * s, min(64 * s + 64, n)):
            acc = acc + float(u[i]) * float(v[i])
        sig.append(acc)
    P = 1
    while P < ns:
        P *= 2
    t = sig + [0.0] * (P - ns)
    h = P // 2
    while h >= 1:
        for j in range(h):
            t[j] = t[j] + t[j + h]
        h //= 2
    return t[0], ns, P


@pytest.mark.parametrize("n, ns, P", [(1, 1, 1), (63, 1, 1), (64, 1, 1), (65, 2, 2), (257, 5, 8), (1024, 16, 16)])
def test_segdot_against_a_hand_written_loop(n, ns, P):
    rng = np.random.default_rng(n)
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    want, hs, hp = hand_dot(u, v)
    assert (hs, hp) == (ns, P)
    got = dsr.segdot(u, v)
    assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64)
    # columns: each its own dot
    U, V = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    got = dsr.segdot(U, V)
    assert bits(got) == bits([hand_dot(U[:, c], V[:, c])[0] for c in range(3)])
    # the order matters at this size: the plain sum differs somewhere, or the segment order is not under test
    if n == 1024:
        assert any(np.float64(dsr.segdot(a, a)).view(np.uint64) != np.float64(np.dot(a, a)).view(np.uint64)
                   for a in rng.standard_normal((20, n)))


def same(a, b):
    """(f, iterations, residual, converged) of two solves, f in bits."""
    assert bits(a[0]) == bits(b[0])
    assert (int(a[1]), bool(a[3])) == (int(b[1]), bool(b[3]))
    assert np.float64(a[2]).view(np.uint64) == np.float64(b[2]).view(np.uint64)


def test_two_nodes_in_closed_form():
    # S = [[0, 1], [1, 0]], y = (1, 0): f* = (1, alpha) / (1 + alpha); CG on a 2 x 2 system ends in two iterations
    p, c, S = dfr.operator(*csr_of(2, [(0, 1, 3.0)]))
    y = np.array([1.0, 0.0])
    for alpha in (0.5, 0.85):
        got = dsr.solve(p, c, S, y, alpha, 1e-12, 10)
        same(got, dsr.solve_loops(p, c, S, y, alpha, 1e-12, 10))
        assert got[3] and got[1] == 2
        assert got[0] == pytest.approx(np.array([1.0, alpha]) / (1.0 + alpha), abs=1e-15)


def test_a_path_with_an_isolated_node_and_a_seed_on_a_row_without_edges():
    p, c, S = dfr.operator(*csr_of(6, [(0, 1, 1.0), (1, 2, 1.0), (2, 3, 1.0), (3, 4, 1.0)]))   # node 5 has no edge
    for y in (np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.25]), np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.7])):
        for alpha in (0.5, 0.99):
            for tol in (1e-6, 1e-10):
                got = dsr.solve(p, c, S, y, alpha, tol, 50)
                same(got, dsr.solve_loops(p, c, S, y, alpha, tol, 50))
                assert got[3] and got[1] <= 6
                # a row without edges: (I - alpha S) is the identity there, f = (1 - alpha) y
                assert got[0][5] == pytest.approx((1.0 - alpha) * y[5], rel=1e-12)
    # the seed on the row without edges alone: b is an eigenvector, one iteration
    assert dsr.solve(p, c, S, np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.7]), 0.5, 1e-10, 50)[1] == 1


def graph(n, seed):
    return dfr.operator(*csr_of(n, random_graph(n, np.random.default_rng(seed))))


def test_vectorised_and_looped_solve_agree_in_bits():
    for n, seed in ((60, 5), (150, 6)):   # one segment; three segments padded to four
        p, c, S = graph(n, seed)
        rng = np.random.default_rng(seed + 10)
        y = np.zeros(n)
        y[rng.choice(n, 7, replace=False)] = rng.uniform(0.3, 1.0, 7)
        for alpha in dsr.ALPHAS:
            for tol in dsr.TOLS:
                got = dsr.solve(p, c, S, y, alpha, tol, 100)
                same(got, dsr.solve_loops(p, c, S, y, alpha, tol, 100))
                assert got[3] and got[1] >= 3


def test_columns_are_independent_and_freeze():
    n = 150
    p, c, S = dfr.operator(*csr_of(n, random_graph(n - 2, np.random.default_rng(9))))   # the last two nodes have no edge
    rng = np.random.default_rng(19)
    Y = np.zeros((n, 5))
    for b, m in enumerate((1, 3, 10, 0, 0)):   # (the last column is all zero)
        Y[rng.choice(n - 2, m, replace=False), b] = rng.uniform(0.3, 1.0, m)
    Y[n - 1, 3] = 0.6                          # a seed on a row without edges alone: one iteration
    F, it, res, conv = dsr.solve(p, c, S, Y, 0.85, 1e-10, 100)
    assert len(set(it.tolist())) >= 3
    for b in range(5):
        same((F[:, b], it[b], res[b], conv[b]), dsr.solve(p, c, S, Y[:, b], 0.85, 1e-10, 100))
    Y2 = Y.copy()
    Y2[:, 1:] = rng.standard_normal((n, 4))
    F2, it2, res2, conv2 = dsr.solve(p, c, S, Y2, 0.85, 1e-10, 100)
    same((F2[:, 0], it2[0], res2[0], conv2[0]), (F[:, 0], it[0], res[0], conv[0]))


def test_a_zero_column_max_iters_and_alpha_zero():
    n = 150
    p, c, S = graph(n, 11)
    rng = np.random.default_rng(21)
    y = np.zeros(n)
    y[rng.choice(n, 9, replace=False)] = rng.uniform(0.3, 1.0, 9)
    for fn in (dsr.solve, dsr.solve_loops):
        f, it, res, conv = fn(p, c, S, np.zeros(n), 0.85, 1e-8, 100)
        assert (it, res, conv) == (0, 0.0, True) and bits(f) == bits(np.zeros(n))
    # max_iters = 3: the third iterate, not converged; it is the prefix of the longer run
    f3, it3, res3, conv3 = dsr.solve(p, c, S, y, 0.85, 1e-10, 3)
    same((f3, it3, res3, conv3), dsr.solve_loops(p, c, S, y, 0.85, 1e-10, 3))
    assert (it3, conv3) == (3, False) and res3 > 1e-10
    full = dsr.solve(p, c, S, y, 0.85, 1e-10, 100)
    assert full[1] > 3 and bits(full[0]) != bits(f3)
    assert bits(dsr.solve(p, c, S, y, 0.85, 1e-300, 3)[0]) == bits(f3)   # (the iterate does not depend on tol)
    # alpha = 0: q = p, a = 1, x = b = y after one iteration
    for fn in (dsr.solve, dsr.solve_loops):
        f, it, res, conv = fn(p, c, S, y, 0.0, 1e-8, 100)
        assert (it, conv) == (1, True) and res == 0.0 and bits(f) == bits(y)


def test_the_residual_reported_is_the_recurrence_residual():
    n = 150
    p, c, S = graph(n, 13)
    Sd = dsr.dense_operator(p, c, S)
    rng = np.random.default_rng(23)
    y = np.zeros(n)
    y[rng.choice(n, 9, replace=False)] = rng.uniform(0.3, 1.0, 9)
    for alpha in dsr.ALPHAS:
        for tol in dsr.TOLS:
            f, it, res, conv = dsr.solve(p, c, S, y, alpha, tol, 200)
            b = (1.0 - alpha) * y
            true = np.linalg.norm(b - (f - alpha * Sd @ f)) / np.linalg.norm(b)
            assert conv and res <= tol and true <= 2.0 * tol
            star = np.linalg.solve(np.eye(n) - alpha * Sd, b)
            assert np.linalg.norm(f - star) <= 2.0 * tol * np.linalg.norm(b) / (1.0 - alpha)


def test_python_validators_run_before_a_handle_is_touched():
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    assert A._diffuse_solve_params(0.0, 1e-8, 1) == (0.0, 1e-8, 1)
    assert A._diffuse_solve_params(0.99, 1.0, np.int64(1024)) == (0.99, 1.0, 1024)
    for alpha, tol, mi in ((-0.1, 1e-8, 10), (1.0, 1e-8, 10), (1.5, 1e-8, 10), (float("nan"), 1e-8, 10), (0.5, 0.0, 10), (0.5, -1e-8, 10),
                           (0.5, float("inf"), 10), (0.5, float("nan"), 10), (0.5, 1e-8, 0), (0.5, 1e-8, 1025), (0.5, 1e-8, -1),
                           (0.5, 1e-8, 2.0), (0.5, 1e-8, True), (0.5, 1e-8, "3")):
        with pytest.raises(ValueError):
            A._diffuse_solve_params(alpha, tol, mi)
    info = A._solve_info(np.array([3, 0], dtype=np.int32), np.array([0.5, np.nan]), np.array([1, 0], dtype=np.int32), False)
    assert info["iterations"].tolist() == [3, 0] and info["converged"].tolist() == [True, False] and info["residual"][0] == 0.5
    assert A._solve_info(np.array([3], dtype=np.int32), np.array([0.5]), np.array([2], dtype=np.int32), True) == \
        {"iterations": 3, "residual": 0.5, "converged": False}
    for name in ("search_diffuse_solve", "search_batch_diffuse_solve", "score_diffuse_solve", "score_diffuse_solve_batch", "diffuse_solve",
                 "diffuse_solve_counters"):
        assert callable(getattr(A, name))
    import inspect
    sig = inspect.signature(A.search_diffuse_solve)
    assert (sig.parameters["tol"].default, sig.parameters["max_iters"].default, sig.parameters["with_info"].default) == (1e-8, 100, False)
    # the C entries are bound
    for sym in ("as_search_diffuse_solve", "as_search_diffuse_solve_batch", "as_score_diffuse_solve_batch", "as_diffuse_solve_seeds",
                "as_diffuse_solve_counters", "as_diffuse_solve_kernel_us"):
        assert getattr(asp._L, sym) is not None
