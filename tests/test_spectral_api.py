"""CPU: what `ArrowSpace.eigsh` refuses before a handle is touched (the refusals that need a graph -- fewer rows than the block,
the "spectral_mib" budget, a feature-mode graph -- are in tests/test_gpu_spectral.py), the bound C entries, and the host
eigensolver of the driver, `as_sym_eig_host` (a cyclic Jacobi; it needs no GPU), against numpy.linalg.eigh: every eigenvalue
within 1e-13 |A|, |A V - V L| and |V^T V - I| within 1e-13 n |A| (2-norms)."""
import inspect

import numpy as np
import pytest


def sym_eig(asp, A):
    n = A.shape[0]
    A = np.ascontiguousarray(A, dtype=np.float64)
    w, V = np.empty(n), np.empty((n, n))
    sweeps = asp._L.as_sym_eig_host(A.ctypes.data, n, w.ctypes.data, V.ctypes.data)
    return sweeps, w, V


def check(asp, A, what):
    n = A.shape[0]
    norm = np.linalg.norm(A, 2)
    sweeps, w, V = sym_eig(asp, A)
    want = np.linalg.eigh(A)[0]
    print(f"{what}: n {n}, {sweeps} sweeps, |w - eigh| / |A| {np.abs(w - want).max() / norm:.2e}, "
          f"|A V - V L| / (n |A|) {np.linalg.norm(A @ V - V * w[None, :], 2) / (n * norm):.2e}, "
          f"|V^T V - I| / (n |A|) {np.linalg.norm(V.T @ V - np.eye(n), 2) / (n * norm):.2e}")
    assert 0 <= sweeps < 64
    assert (np.diff(w) >= 0.0).all()
    assert (np.abs(w - want) <= 1e-13 * norm).all()
    assert np.linalg.norm(A @ V - V * w[None, :], 2) <= 1e-13 * n * norm
    assert np.linalg.norm(V.T @ V - np.eye(n), 2) <= 1e-13 * n * norm
    return w, V


def orthogonal(n, rng):
    return np.linalg.qr(rng.standard_normal((n, n)))[0]


@pytest.mark.parametrize("n", [16, 64])
def test_sym_eig_on_random_symmetric_matrices(n):
    import pyarrowspace_amd as asp
    rng = np.random.default_rng(n)
    for _ in range(3):
        A = rng.standard_normal((n, n))
        check(asp, A + A.T, "random symmetric")


@pytest.mark.parametrize("n", [16, 64])
def test_sym_eig_on_a_gram_matrix_of_condition_1e12(n):
    import pyarrowspace_amd as asp
    rng = np.random.default_rng(100 + n)
    X = orthogonal(4 * n, rng)[:, :n] * np.logspace(0.0, -6.0, n)[None, :] @ orthogonal(n, rng)
    G = X.T @ X
    assert 1e11 <= np.linalg.cond(G) <= 1e13 and np.linalg.norm(G, 2) >= 0.99
    w, V = check(asp, G, "Gram, condition 1e12")
    # the Jacobi keeps the small eigenvalues of a positive definite matrix: the driver divides by their roots
    assert (w > 0.0).all() and w[0] == pytest.approx(1e-12, rel=1e-3)


def test_sym_eig_on_a_nineteen_fold_eigenvalue():
    import pyarrowspace_amd as asp
    rng = np.random.default_rng(19)
    Q = orthogonal(64, rng)
    lam = np.concatenate([np.ones(19), rng.uniform(-1.0, 0.9, 45)])
    A = (Q * lam[None, :]) @ Q.T
    w, V = check(asp, 0.5 * (A + A.T), "a 19-fold eigenvalue")
    assert (np.abs(w[-19:] - 1.0) <= 1e-13).all() and w[-20] <= 0.9 + 1e-13
    # the eigenvectors of the cluster span the right space
    P = V[:, -19:] @ V[:, -19:].T
    assert np.linalg.norm(P - Q[:, :19] @ Q[:, :19].T, 2) <= 1e-12


def test_sym_eig_edge_cases():
    import pyarrowspace_amd as asp
    sweeps, w, V = sym_eig(asp, np.array([[3.0]]))
    assert (sweeps, w.tolist(), V.tolist()) == (0, [3.0], [[1.0]])
    sweeps, w, V = sym_eig(asp, np.zeros((4, 4)))
    assert sweeps == 0 and (w == 0.0).all() and (V == np.eye(4)).all()
    sweeps, w, V = sym_eig(asp, np.diag([2.0, -1.0, 0.5]))
    assert sweeps <= 1 and w.tolist() == [-1.0, 0.5, 2.0] and (np.abs(V) == np.eye(3)[:, [1, 2, 0]]).all()
    check(asp, np.array([[0.0, 1.0], [1.0, 0.0]]), "a zero diagonal")
    assert asp._L.as_sym_eig_host(None, 4, w.ctypes.data, V.ctypes.data) == -1
    assert asp._L.as_sym_eig_host(w.ctypes.data, 0, w.ctypes.data, V.ctypes.data) == -1


def test_python_validators_run_before_a_handle_is_touched():
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    assert A._eigsh_params(1, 1e-8, 200, 16, 0) == (1, 1e-8, 200, 16, 0, 16)
    assert A._eigsh_params(12, 0.5, 1, 1, 2 ** 63 - 1) == (12, 0.5, 1, 1, 2 ** 63 - 1, 16)
    assert A._eigsh_params(np.int64(13), 1e-12, 10000, 64, 5) == (13, 1e-12, 10000, 64, 5, 64)
    assert A._eigsh_params(48, 1e-8, 200, 16, 0)[5] == 64
    good = {"m": 8, "tol": 1e-8, "max_iters": 200, "degree": 16, "seed": 0}
    for key, bad in (("m", (0, 49, -1, 2.0, True, "3", None)), ("tol", (0.0, 1.0, -1e-8, 1.5, float("inf"), float("nan"))),
                     ("max_iters", (0, 10001, -1, 2.0, True)), ("degree", (0, 65, -1, 2.0, True)), ("seed", (-1, 2 ** 63, 1.0, True))):
        for v in bad:
            with pytest.raises(ValueError, match=key):
                A._eigsh_params(**{**good, key: v})
    sig = inspect.signature(A.eigsh)
    assert [sig.parameters[k].default for k in ("tol", "max_iters", "degree", "seed", "with_info")] == [1e-8, 200, 16, 0, False]
    with pytest.raises(TypeError):
        A.eigsh(object.__new__(A), None, 3)   # (the graph is checked before the handle is used)
    for name in ("eigsh", "eigsh_counters", "_spectral_op"):
        assert callable(getattr(A, name))
    for sym in ("as_graph_eigs", "as_graph_eigs_counters", "as_graph_eigs_kernel_us", "as_spectral_op", "as_sym_eig_host"):
        assert getattr(asp._L, sym) is not None
    assert asp._L.as_set_tuning(b"spectral_mib", 0) == 0
