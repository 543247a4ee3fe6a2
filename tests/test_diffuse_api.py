"""CPU: the numpy reference of graph diffusion (tests/diffuse_ref.py) on hand-built graphs, its limits and its
column independence, and the Python validators of the diffusion forms that run before a handle is touched."""
import numpy as np
import pytest

import diffuse_ref as dfr


def csr_of(n, edges):
    """to_csr()'s layout of a symmetric weighted graph: L = I - D^-1/2 A D^-1/2, the diagonal stored (1, or 0 for a node
    without an edge), columns ascending."""
    A = np.zeros((n, n))
    for i, j, w in edges:
        A[i, j] = A[j, i] = w
    deg = A.sum(axis=1)
    indptr, indices, values = [0], [], []
    for i in range(n):
        for j in range(n):
            if i == j:
                indices.append(j)
                values.append(1.0 if deg[i] > 0 else 0.0)
            elif A[i, j] != 0.0:
                indices.append(j)
                values.append(-A[i, j] / np.sqrt(deg[i] * deg[j]))
        indptr.append(len(indices))
    return np.array(indptr), np.array(indices), np.array(values)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def test_operator_drops_the_diagonal_and_flips_the_sign():
    ip, ix, v = csr_of(4, [(0, 1, 2.0), (1, 2, 1.0)])   # node 3 has no edge
    p, c, S = dfr.operator(ip, ix, v)
    assert p.tolist() == [0, 1, 3, 4, 4]
    assert c.tolist() == [1, 0, 2, 1]
    assert S.tolist() == [2.0 / np.sqrt(2.0 * 3.0), 2.0 / np.sqrt(3.0 * 2.0), 1.0 / np.sqrt(3.0 * 1.0), 1.0 / np.sqrt(1.0 * 3.0)]


def test_two_nodes_in_closed_form():
    # S = [[0, 1], [1, 0]]: f(t+1) = alpha swap(f(t)) + (1 - alpha) y; with y = (1, 0) and alpha = 1/2 every value is a dyadic
    # fraction: f(1) = (1/2, 1/2), f(2) = (3/4, 1/4), f(3) = (5/8, 3/8)
    p, c, S = dfr.operator(*csr_of(2, [(0, 1, 3.0)]))
    assert S.tolist() == [1.0, 1.0]
    y = np.array([1.0, 0.0])
    want = {0: [1.0, 0.0], 1: [0.5, 0.5], 2: [0.75, 0.25], 3: [0.625, 0.375]}
    for t, w in want.items():
        assert dfr.diffuse(p, c, S, y, 0.5, t).tolist() == w
        assert dfr.diffuse_loops(p, c, S, y, 0.5, t).tolist() == w
    # the fixed point (1 - a) (I - a S)^-1 y = (1, a) / (1 + a)
    f = dfr.diffuse(p, c, S, y, 0.5, 64)
    assert f == pytest.approx([2.0 / 3.0, 1.0 / 3.0], abs=1e-15)


def test_a_path_of_five_and_an_isolated_node():
    p, c, S = dfr.operator(*csr_of(6, [(0, 1, 1.0), (1, 2, 1.0), (2, 3, 1.0), (3, 4, 1.0)]))   # node 5 has no edge
    y = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.25])
    r = 1.0 / np.sqrt(2.0)
    f1 = dfr.diffuse(p, c, S, y, 0.5, 1)
    # one step reaches node 1 only: S_10 = 1 / sqrt(1 * 2); the isolated node keeps (1 - alpha) y
    assert f1.tolist() == [0.5, 0.5 * (r * 1.0), 0.0, 0.0, 0.0, 0.5 * 0.25]
    for steps in (0, 1, 2, 7):
        f = dfr.diffuse(p, c, S, y, 0.5, steps)
        assert bits(f) == bits(dfr.diffuse_loops(p, c, S, y, 0.5, steps))
        assert (f[min(steps, 4) + 1:5] == 0.0).all()        # step t reaches t nodes down the path
        assert f[5] == (0.25 if steps == 0 else 0.125)      # a row without edges contributes nothing and receives nothing


def random_graph(n, rng, extra=3):
    edges = {}
    for i in range(1, n):
        edges[(int(rng.integers(0, i)), i)] = float(rng.uniform(0.1, 1.0))
    for _ in range(extra * n):
        i, j = sorted(int(v) for v in rng.integers(0, n, 2))
        if i != j:
            edges[(i, j)] = float(rng.uniform(0.1, 1.0))
    return [(i, j, w) for (i, j), w in edges.items()]


def test_alpha_zero_and_no_steps_return_the_seeds_bits():
    rng = np.random.default_rng(3)
    p, c, S = dfr.operator(*csr_of(40, random_graph(40, rng)))
    y = np.zeros(40)
    y[[3, 9, 11, 30]] = [0.7, -0.2, -0.0, 1e-300]
    assert bits(dfr.diffuse(p, c, S, y, 0.85, 0)) == bits(y)
    for steps in (1, 5):
        assert bits(dfr.diffuse(p, c, S, y, 0.0, steps) + 0.0) == bits(y + 0.0)   # (alpha = 0: 0 acc + y; the sign of a zero is free)


def test_vectorised_and_looped_reference_agree_in_bits():
    rng = np.random.default_rng(5)
    p, c, S = dfr.operator(*csr_of(60, random_graph(60, rng)))
    y = np.zeros(60)
    y[rng.choice(60, 7, replace=False)] = rng.standard_normal(7)
    for steps in (0, 1, 2, 7):
        for alpha in (0.5, 0.99):
            assert bits(dfr.diffuse(p, c, S, y, alpha, steps)) == bits(dfr.diffuse_loops(p, c, S, y, alpha, steps))


def test_convergence_to_the_fixed_point():
    # |f(t) - f*| <= alpha^t |y - f*| in the D^1/2-weighted norm in which S is a contraction; 2 alpha^t max|y| / (1 - alpha)
    # bounds it with room for the weights on this graph (degrees within a factor of a few)
    rng = np.random.default_rng(7)
    n, alpha = 200, 0.85
    ip, ix, v = csr_of(n, random_graph(n, rng))
    p, c, S = dfr.operator(ip, ix, v)
    Sd = np.zeros((n, n))
    for i in range(n):
        Sd[i, c[p[i]:p[i + 1]]] = S[p[i]:p[i + 1]]
    y = np.zeros(n)
    y[rng.choice(n, 10, replace=False)] = rng.uniform(0.2, 1.0, 10)
    star = np.linalg.solve(np.eye(n) - alpha * Sd, (1.0 - alpha) * y)
    for steps in (10, 40, 64):
        err = float(np.abs(dfr.diffuse(p, c, S, y, alpha, steps) - star).max())
        bound = 2.0 * alpha ** steps * float(np.abs(y).max()) / (1.0 - alpha)
        print(f"steps {steps}: error {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (steps, err, bound)


def test_columns_are_independent():
    rng = np.random.default_rng(9)
    p, c, S = dfr.operator(*csr_of(50, random_graph(50, rng)))
    Y = np.zeros((50, 5))
    for b in range(5):
        Y[rng.choice(50, 4, replace=False), b] = rng.standard_normal(4)
    F = dfr.diffuse(p, c, S, Y, 0.7, 6)
    for b in range(5):
        assert bits(F[:, b]) == bits(dfr.diffuse(p, c, S, Y[:, b], 0.7, 6))
    Y2 = Y.copy()
    Y2[:, 1:] = rng.standard_normal((50, 4))
    assert bits(dfr.diffuse(p, c, S, Y2, 0.7, 6)[:, 0]) == bits(F[:, 0])


def test_rank_orders_by_value_then_index_and_ignores_the_sign_of_zero():
    f = np.array([0.0, 0.5, -0.0, 0.5, -1.0])
    assert dfr.rank(f, None, 4) == [(1, 0.5), (3, 0.5), (0, 0.0), (2, 0.0)]
    assert dfr.rank(f, [4, 2, 0, 2], 9) == [(0, 0.0), (2, 0.0), (4, -1.0)]


def test_python_validators_run_before_a_handle_is_touched():
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    assert A._diffuse_params(0.0, 0) == (0.0, 0) and A._diffuse_params(0.99, np.int64(64)) == (0.99, 64)
    for alpha, steps in ((-0.1, 3), (1.0, 3), (1.5, 3), (float("nan"), 3), (0.5, -1), (0.5, 65), (0.5, 2.0), (0.5, True), (0.5, "3")):
        with pytest.raises(ValueError):
            A._diffuse_params(alpha, steps)
    ids, vals, offs = A._diffuse_seeds([([4, 1], [0.5, -0.0]), ([], []), (np.array([2], dtype=np.uint8), [1.0])], 5)
    assert ids.tolist() == [4, 1, 2] and ids.dtype == np.int64 and bits(vals) == bits([0.5, -0.0, 1.0]) and offs.tolist() == [0, 2, 2, 3]
    assert [a.tolist() for a in A._diffuse_seeds([], 5)] == [[], [], [0]]
    for bad in ([([1, 1], [0.1, 0.2])], [([5], [0.1])], [([-1], [0.1])], [([1], [float("inf")])], [([1], [float("nan")])],
                [([1, 2], [0.1])], [([[1]], [[0.1]])], [3]):
        with pytest.raises(ValueError):
            A._diffuse_seeds(bad, 5)
    for bad in ([([1.0], [0.1])], [([True, False, False, False, False], [0.1] * 5)]):
        with pytest.raises(TypeError):
            A._diffuse_seeds(bad, 5)
    for name in ("search_diffuse", "search_batch_diffuse", "score_diffuse", "score_diffuse_batch", "diffuse", "diffuse_counters"):
        assert callable(getattr(A, name))
    import arrowspace
    assert arrowspace.ArrowSpace is A
