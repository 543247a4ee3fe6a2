"""Reference of graph eigenpairs in numpy fp64, for the tests and tools/spectral_bench.py: the four device
primitives with the SPEC's order and roundings (`step`, `gram`, `rotate`, `colnorm2`; each `*_loops` is the SPEC word for word as
plain Python loops, for small blocks), the start block (`start_block`) and the driver (`eigs`: block Chebyshev-filtered subspace
iteration with Rayleigh-Ritz, LAPACK's `eigh` in the place of the library's Jacobi, so its output is close to the device's and
not equal in bits).  The operator and a row's sum are tests/diffuse_ref.py's and tests/diffuse_solve_ref.py's (`operator`,
`RowSums`), the column reduction is S20's `segdot`."""
import math

import numpy as np

import diffuse_solve_ref as dsr

GRAM_SEG = 1024          # rows of a segment of S21's Gram
LO = -1.0                # the lower end of S's spectrum (tests/test_diffuse_solve_inputs.py)
GAP_FLOOR = 1e-3         # cut stays this share of (theta_1 - lo) below theta_1
GROWTH = 2.0e6           # the filter's amplification of theta_1 over the damped interval, at most
BREAKDOWN = 1e-14        # a Gram eigenvalue <= this times the largest: the block has lost a direction
M_MAX = 48
U64 = (1 << 64) - 1
# the solver cases of tests/test_gpu_spectral.py, (m, C), on both shapes of diffuse_ref.SHAPES, at TOL within MAX_ITERS
CASES = ((1, 16), (8, 16), (12, 16), (13, 64), (19, 64), (48, 64))
# the solver cases of tests/test_gpu_diffusion_scale.py on shape C of diffuse_ref.SCALE_SHAPES (the eigenvalue 1 has multiplicity 19)
SCALE_CASES = ((8, 16), (13, 64), (19, 64), (48, 64))
TOL = 1e-8
MAX_ITERS = 60
# max |V V^T - I| of this reference over those cases stays below this (tests/test_spectral_inputs.py prints and asserts it: the
# largest seen is 2.9e-15); the device's bound is 100 times it, since the Jacobi's rounding differs from LAPACK's
ORTHO_DEFECT = 3e-15


def hand_block(n, C, seed):
    """A block [n, C] of mixed sign and magnitudes 1e-8 .. 1e8: a changed order of a sum changes its bits."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, C)) * 10.0 ** rng.uniform(-8.0, 8.0, (n, C))


def block_width(m):
    return 16 if m <= 12 else 64


def start_block(n, C, seed):
    """The start block [n, C]: splitmix64's finaliser over (i C + c) 0x9E3779B97F4A7C15 + seed 0xBF58476D1CE4E5B9 (mod 2^64),
    the top 53 bits as a number of [-0.5, 0.5)."""
    with np.errstate(over="ignore"):
        x = np.arange(n * C, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((seed * 0xBF58476D1CE4E5B9) & U64)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return ((x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5).reshape(n, C)


def start_block_loops(n, C, seed):
    out = np.empty((n, C))
    for i in range(n):
        for c in range(C):
            x = ((i * C + c) * 0x9E3779B97F4A7C15 + seed * 0xBF58476D1CE4E5B9) & U64
            x ^= x >> 30
            x = (x * 0xBF58476D1CE4E5B9) & U64
            x ^= x >> 27
            x = (x * 0x94D049BB133111EB) & U64
            x ^= x >> 31
            out[i, c] = float(x >> 11) * 2.0 ** -53 - 0.5
    return out


def step(rows, V, a, b, g=0.0, W=None):
    """S21's step: fl(fl(fl(a acc) + fl(b V)) + fl(g W)), acc = `rows`(V) (a `RowSums`); g == 0: W is not read, the last term
    is absent."""
    out = a * rows(V) + b * V
    if g != 0.0:
        out = out + g * W
    return out


def step_loops(indptr, indices, S, V, a, b, g=0.0, W=None):
    n, C = V.shape
    out = np.empty((n, C))
    for i in range(n):
        for c in range(C):
            acc = 0.0
            for e in range(int(indptr[i]), int(indptr[i + 1])):
                acc = acc + float(S[e]) * float(V[int(indices[e]), c])
            v = a * acc + b * float(V[i, c])
            if g != 0.0:
                v = v + g * float(W[i, c])
            out[i, c] = v
    return out


def _tree(t):
    """S20's halving tree over the leading axis (padded to a power of two with +0.0)."""
    ns = t.shape[0]
    P = 1
    while P < ns:
        P *= 2
    pad = np.zeros((P,) + t.shape[1:])
    pad[:ns] = t
    h = P // 2
    while h >= 1:
        pad = pad[:h] + pad[h:2 * h]
        h //= 2
    return pad[0]


def gram(A, B):
    """S21's Gram [C, C]: G[i][j] = sum_r A[r][i] B[r][j] -- per segment of 1 024 rows a partial from +0.0 in ascending r, then the
    halving tree over the segments."""
    n, C = A.shape
    ns = -(-n // GRAM_SEG)
    part = np.zeros((ns, C, C))
    for s in range(ns):
        acc = np.zeros((C, C))
        for r in range(s * GRAM_SEG, min((s + 1) * GRAM_SEG, n)):
            acc = acc + A[r][:, None] * B[r][None, :]
        part[s] = acc
    return _tree(part)


def gram_loops(A, B):
    """(A [n, Ca] and B [n, Cb] -> [Ca, Cb]: a few columns of either give a few rows or columns of the Gram at a large n)"""
    n = A.shape[0]
    ns = -(-n // GRAM_SEG)
    P = 1
    while P < ns:
        P *= 2
    G = np.empty((A.shape[1], B.shape[1]))
    for i in range(A.shape[1]):
        for j in range(B.shape[1]):
            t = []
            for s in range(ns):
                acc = 0.0
                for r in range(s * GRAM_SEG, min((s + 1) * GRAM_SEG, n)):
                    acc = acc + float(A[r, i]) * float(B[r, j])
                t.append(acc)
            t += [0.0] * (P - ns)
            h = P // 2
            while h >= 1:
                for q in range(h):
                    t[q] = t[q] + t[q + h]
                h //= 2
            G[i, j] = t[0]
    return G


def rotate(X, T):
    """S21's rotate: out[r][j] = sum_k X[r][k] T[k][j], k ascending from +0.0."""
    out = np.zeros((X.shape[0], T.shape[1]))
    for k in range(T.shape[0]):
        out = out + X[:, k][:, None] * T[k][None, :]
    return out


def rotate_loops(X, T):
    n, C = X.shape
    out = np.empty((n, T.shape[1]))
    for r in range(n):
        for j in range(T.shape[1]):
            acc = 0.0
            for k in range(C):
                acc = acc + float(X[r, k]) * float(T[k, j])
            out[r, j] = acc
    return out


def colnorm2(X, Y, theta):
    """S21's colnorm2 [C]: S20's segdot of R = fl(Y - fl(X theta_c)) with itself, column by column."""
    R = Y - X * np.asarray(theta, dtype=np.float64)[None, :]
    return dsr.segdot(R, R)


def colnorm2_loops(X, Y, theta):
    n, C = X.shape
    ns = -(-n // dsr.SEG)
    P = 1
    while P < ns:
        P *= 2
    out = np.empty(C)
    for c in range(C):
        t = []
        for s in range(ns):
            acc = 0.0
            for r in range(s * dsr.SEG, min((s + 1) * dsr.SEG, n)):
                d = float(Y[r, c]) - float(X[r, c]) * float(theta[c])
                acc = acc + d * d
            t.append(acc)
        t += [0.0] * (P - ns)
        h = P // 2
        while h >= 1:
            for q in range(h):
                t[q] = t[q] + t[q + h]
            h //= 2
        out[c] = t[0]
    return out


def filter_plan(theta, degree):
    """The filter's scalars from the Ritz values (descending): (e, c, d) -- the damped interval [lo, cut] has half-width e and
    centre c, d steps."""
    t1, tc = float(theta[0]), float(theta[-1])
    cut = min(tc, t1 - GAP_FLOOR * (t1 - LO))
    cut = max(cut, LO + GAP_FLOOR * (t1 - LO))   # (a Ritz value at lo itself: the interval keeps a width)
    e = (cut - LO) / 2.0
    c = (cut + LO) / 2.0
    tt = (t1 - c) / e
    d = max(1, int(min(float(degree), math.floor(math.log(GROWTH) / math.acosh(tt)))))
    return e, c, d


def orthonormalise(X, counts):
    """X (U Lambda^-1/2) of X^T X = U Lambda U^T; None on a breakdown."""
    G = gram(X, X)
    counts["gram"] += 1
    lam, U = np.linalg.eigh(G)
    if not lam.min() > BREAKDOWN * lam.max():
        return None
    counts["rotate"] += 1
    return rotate(X, U / np.sqrt(lam)[None, :])


def sign_rule(V):
    """Rows of V: the entry of largest magnitude (lowest index on ties) made positive."""
    V = V.copy()
    for j in range(V.shape[0]):
        if V[j, int(np.argmax(np.abs(V[j])))] < 0.0:
            V[j] = -V[j]
    return V


def eigs(indptr, indices, S, m, tol=1e-8, max_iters=200, degree=16, seed=0):
    """S21's driver -> (values [m] descending, vectors [m, n], info) with info = {"iterations", "residuals" [m], "converged",
    "filter_steps", "block", "gram", "rotate"}; raises RuntimeError on a breakdown."""
    n = len(indptr) - 1
    C = block_width(m)
    rows = dsr.RowSums(indptr, indices, S)
    counts = {"gram": 0, "rotate": 0}
    steps = 0
    X = start_block(n, C, seed)
    for _ in range(2):
        X = orthonormalise(X, counts)
        if X is None:
            raise RuntimeError("eigs: the start block lost a direction")
    it, conv = 0, False
    while True:
        it += 1
        Y = step(rows, X, 1.0, 0.0)
        steps += 1
        H = gram(X, Y)
        counts["gram"] += 1
        H = 0.5 * (H + H.T)
        th, Q = np.linalg.eigh(H)
        th, Q = th[::-1].copy(), np.ascontiguousarray(Q[:, ::-1])
        X, Y = rotate(X, Q), rotate(Y, Q)
        counts["rotate"] += 2
        res = np.sqrt(colnorm2(X, Y, th))
        conv = bool((res[:m] <= tol).all())
        if conv or it >= max_iters:
            break
        e, c, d = filter_plan(th, degree)
        Zp, Z = X, step(rows, X, 1.0 / e, -c / e)
        for _ in range(d - 1):
            Zp, Z = Z, step(rows, Z, 2.0 / e, -2.0 * c / e, -1.0, Zp)
        steps += d
        X = Z
        for _ in range(2):
            X = orthonormalise(X, counts)
            if X is None:
                raise RuntimeError(f"eigs: the block lost a direction in iteration {it}")
    info = {"iterations": it, "residuals": res[:m].copy(), "converged": conv, "filter_steps": steps, "block": C, **counts}
    return th[:m].copy(), sign_rule(X[:, :m].T), info
