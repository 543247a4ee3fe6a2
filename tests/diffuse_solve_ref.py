"""Reference of fixed-point diffusion search in numpy fp64, for the tests and tools/diffuse_solve_bench.py:
conjugate gradients on (I - alpha S) f = (1 - alpha) y with the SPEC's one reduction (`segdot`: 64-row segments in row order, then
a halving tree), every column on its own (`solve`; `solve_loops` is the SPEC word for word as Python loops, for the hand-built
graphs).  The operator, the seeds and the ranking are tests/diffuse_ref.py's (`operator`, `seeds_vector`, `rank`, `canon`), and a
row's sum runs in the order of `diffuse_ref.diffuse`: one pass per edge rank."""
import numpy as np

SEG = 64
ALPHAS = (0.5, 0.85, 0.99)
TOLS = (1e-6, 1e-10)
NCOL = 70   # seed columns of the fixtures: a 64-wide chunk and a 16-wide one for the remaining six


def segdot(u, v):
    """S20's dot of [n] (-> a float) or [n, C] (-> [C], every column on its own) arrays."""
    prod = np.asarray(u, dtype=np.float64) * np.asarray(v, dtype=np.float64)
    n = prod.shape[0]
    ns = -(-n // SEG)
    P = 1
    while P < ns:
        P *= 2
    # rows past n count as +0.0 products: sigma + (+0.0) == sigma (sigma starts at +0.0 and so is never -0.0)
    pad = np.zeros((P * SEG,) + prod.shape[1:])
    pad[:n] = prod
    pad = pad.reshape((P, SEG) + prod.shape[1:])
    t = np.zeros((P,) + prod.shape[1:])
    for j in range(SEG):
        t = t + pad[:, j]
    h = P // 2
    while h >= 1:
        t = t[:h] + t[h:2 * h]
        h //= 2
    return t[0]


class RowSums:
    """acc = S p with every row summed in CSR order: the edge-rank passes of `diffuse_ref.diffuse`, planned once."""

    def __init__(self, indptr, indices, S):
        self.indptr = np.asarray(indptr, dtype=np.int64)
        self.indices = np.asarray(indices, dtype=np.int64)
        self.S = np.asarray(S, dtype=np.float64)
        deg = np.diff(self.indptr)
        self.order = np.argsort(-deg, kind="stable")   # rows by descending degree: those with degree > r are a prefix
        self.counts = np.searchsorted(-deg[self.order], -np.arange(int(deg.max()) if deg.size else 0), side="left")

    def __call__(self, f):
        acc = np.zeros_like(f)
        for r in range(len(self.counts)):
            rows = self.order[:self.counts[r]]
            e = self.indptr[rows] + r
            s = self.S[e] if f.ndim == 1 else self.S[e][:, None]
            acc[rows] = acc[rows] + s * f[self.indices[e]]
        return acc


def solve(indptr, indices, S, y, alpha, tol, max_iters):
    """S20 for y [n] or [n, C] -> (f, iterations, residual, converged), the last three scalars or [C] arrays.  A column that has
    stopped is taken out of the arrays the arithmetic runs over, so no column sees another."""
    y = np.asarray(y, dtype=np.float64)
    one = y.ndim == 1
    Y = y.reshape(y.shape[0], -1)
    n, C = Y.shape
    rows = RowSums(indptr, indices, S)
    om = 1.0 - alpha
    x = np.zeros((n, C))
    r = om * Y
    p = r.copy()
    rho = segdot(r, r).reshape(C)
    bb = rho.copy()
    theta = (tol * tol) * bb
    iters = np.zeros(C, dtype=np.int64)
    conv = bb == 0.0
    live = np.flatnonzero(~conv)
    for k in range(1, int(max_iters) + 1):
        if live.size == 0:
            break
        pl = p[:, live]
        q = pl - alpha * rows(pl)
        pi = segdot(pl, q).reshape(-1)
        ok = pi > 0.0                       # (NaN: a breakdown)
        live, pl, q, pi = live[ok], pl[:, ok], q[:, ok], pi[ok]
        if live.size == 0:
            break
        a = rho[live] / pi
        x[:, live] = x[:, live] + a * pl
        rl = r[:, live] - a * q
        r[:, live] = rl
        rho2 = segdot(rl, rl).reshape(-1)
        iters[live] = k
        done = rho2 <= theta[live]
        g = rho2 / rho[live]
        rho[live] = rho2
        conv[live[done]] = True
        go = ~done
        p[:, live[go]] = rl[:, go] + g[go] * pl[:, go]
        live = live[go]
    with np.errstate(invalid="ignore", divide="ignore"):
        res = np.where(bb == 0.0, 0.0, np.sqrt(rho / np.where(bb == 0.0, 1.0, bb)))
    if one:
        return x[:, 0], int(iters[0]), float(res[0]), bool(conv[0])
    return x, iters, res, conv


def solve_loops(indptr, indices, S, y, alpha, tol, max_iters):
    """The SPEC word for word, one column: plain Python loops -> (f, iterations, residual, converged)."""
    n = len(indptr) - 1

    def dot(u, v):
        ns = -(-n // SEG)
        sig = []
        for s in range(ns):
            acc = 0.0
            for i in range(SEG * s, min(SEG * s + SEG, n)):
                acc = acc + u[i] * v[i]
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
        return t[0]

    om = 1.0 - alpha
    b = [om * float(v) for v in y]
    x = [0.0] * n
    r = list(b)
    p = list(b)
    rho = dot(r, r)
    bb = rho
    theta = (tol * tol) * bb
    if bb == 0.0:
        return np.zeros(n), 0, 0.0, True
    iters, conv = 0, False
    for k in range(1, int(max_iters) + 1):
        q = []
        for i in range(n):
            acc = 0.0
            for e in range(int(indptr[i]), int(indptr[i + 1])):
                acc = acc + float(S[e]) * p[int(indices[e])]
            q.append(p[i] - alpha * acc)
        pi = dot(p, q)
        if not pi > 0.0:
            break
        a = rho / pi
        x = [x[i] + a * p[i] for i in range(n)]
        r = [r[i] - a * q[i] for i in range(n)]
        rho2 = dot(r, r)
        iters = k
        if rho2 <= theta:
            rho, conv = rho2, True
            break
        g = rho2 / rho
        p = [r[i] + g * p[i] for i in range(n)]
        rho = rho2
    return np.array(x, dtype=np.float64), iters, float(np.sqrt(rho / bb)), conv


def dense_operator(indptr, indices, S):
    """S as a dense [n, n] array (the small test shapes only)."""
    n = len(indptr) - 1
    Sd = np.zeros((n, n))
    for i in range(n):
        Sd[i, indices[indptr[i]:indptr[i + 1]]] = S[indptr[i]:indptr[i + 1]]
    return Sd


def seed_columns(n, topk, count=NCOL, seed=20):
    """The seed lists of the fixtures: `count` columns of `topk` random items with values in [0.3, 1] -> [(ids, values)]."""
    rng = np.random.default_rng(seed)
    return [(np.sort(rng.choice(n, topk, replace=False)).astype(np.int64), rng.uniform(0.3, 1.0, topk)) for _ in range(count)]
