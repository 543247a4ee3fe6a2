"""Reference of graph diffusion in numpy fp64, for the tests and tools/diffuse_bench.py: the operator S from
`GraphLaplacian.to_csr()` (`operator`), the recurrence with the SPEC's order and roundings (`diffuse`; `diffuse_loops` is the
same as three plain Python loops, for the hand-built graphs) and the ranking of the answer (`rank`)."""
import numpy as np

# the shapes of tests/test_gpu_diffuse.py (and of the CPU check of its inputs): (n, d, nclust, k, topk, metric, kernel)
SHAPES = {"A": (257, 16, 4, 4, 8, "l2", "gaussian"),
          "B": (1000, 24, 16, 8, 15, "cosine", "rational")}
# the shapes of tests/test_gpu_diffusion_scale.py alone, in the same layout: the sizes at which the reductions of S20 and S21 get
# more segments than one trip of their trees takes.  C: 3 Gram segments of 1 024 rows in a tree padded to 4, 33 dot segments of 64,
# a remainder of 5 modulo 16, 64 and 1 024.  L: the smallest n with more than 2 048 dot segments and one row in the last (2 050):
# the 1 024 threads of the solve's tree take a second trip over the 2 048 pairs of its first level, whose upper halves (segments
# 3 072 and up) are all padding.  M: 3 600 dot segments, so that 528 pairs of that second trip add a partial that exists.
SCALE_SHAPES = {"C": (2053, 16, 12, 6, 10, "l2", "gaussian"),
                "L": (131137, 8, 64, 4, 8, "l2", "gaussian"),
                "M": (230337, 8, 64, 4, 8, "l2", "gaussian")}
# rows calibrate_eps samples where its default of 256 is too many: 256 x n distances are about 270 MB per temporary at L's n
EPS_SAMPLE = {"L": 64, "M": 64}
TILE_EDGES = 8   # the "diffuse_tile_edges" the GPU test sets: rows of 3 x 8 edges and more span tiles
TAU = 0.62
NQ = 6


def shape_items(name):
    """(X, graph parameters) of a shape of SHAPES or SCALE_SHAPES: the clustered() / calibrate_eps recipe of
    tests/test_gpu_range.py."""
    from conftest import calibrate_eps, clustered
    n, d, nclust, k, topk, metric, kernel = SHAPES[name] if name in SHAPES else SCALE_SHAPES[name]
    X = clustered(n, d, nclust=nclust)
    eps = calibrate_eps(X, k, metric, sample=EPS_SAMPLE[name]) if name in EPS_SAMPLE else calibrate_eps(X, k, metric)
    gp = {"eps": eps, "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
    return X, gp


def queries_of(X, rng, count, served=None):
    """The query recipe of tests/test_gpu_subset.py; with `served`, only queries it accepts (lambda_q != 0)."""
    n, d = X.shape
    out = []
    while len(out) < count:
        q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        if served is None or served(q):
            out.append(q)
    return out


def operator(indptr, indices, values):
    """S of S19 from `to_csr()`'s (indptr, indices, values): the diagonal dropped, the sign flipped, the order of a row kept.
    -> (indptr, indices, S)."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    values = np.asarray(values, dtype=np.float64)
    n = indptr.shape[0] - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    keep = indices != rows
    out_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=out_ptr[1:])
    return out_ptr, np.ascontiguousarray(indices[keep]), np.ascontiguousarray(-values[keep])


def seeds_vector(n, ids, vals):
    """y of S19: +0.0 but at the seeds; an entry whose value is not finite is left out."""
    y = np.zeros(n)
    for i, v in zip(ids, vals):
        if np.isfinite(v):
            y[int(i)] = v
    return y


def diffuse(indptr, indices, S, y, alpha, steps):
    """f after `steps` steps of S19 from f = y.  y: [n] or [n, C] (every column on its own).  One pass per edge rank r: all rows
    with more than r stored entries add their r-th product at once, so a row's sum keeps the CSR's order; numpy rounds every
    product and every sum once (no FMA)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    y = np.asarray(y, dtype=np.float64)
    deg = np.diff(indptr)
    order = np.argsort(-deg, kind="stable")   # rows by descending degree: those with degree > r are a prefix
    counts = np.searchsorted(-deg[order], -np.arange(int(deg.max()) if deg.size else 0), side="left")
    om = 1.0 - alpha
    oy = om * y
    f = y.copy()
    for _ in range(int(steps)):
        acc = np.zeros_like(f)
        for r in range(len(counts)):
            rows = order[:counts[r]]          # degree > r
            e = indptr[rows] + r
            s = S[e] if f.ndim == 1 else S[e][:, None]
            acc[rows] = acc[rows] + s * f[indices[e]]
        f = alpha * acc + oy
    return f


def diffuse_loops(indptr, indices, S, y, alpha, steps):
    """The SPEC word for word, one column: three Python loops."""
    n = len(indptr) - 1
    om = 1.0 - alpha
    f = [float(v) for v in y]
    for _ in range(int(steps)):
        g = []
        for i in range(n):
            acc = 0.0
            for e in range(int(indptr[i]), int(indptr[i + 1])):
                acc = acc + float(S[e]) * f[int(indices[e])]
            g.append(alpha * acc + om * float(y[i]))
        f = g
    return np.array(f, dtype=np.float64)


def rank(f, ids, k):
    """The first k of `ids` (None: every item) by (f descending, index ascending), -0.0 == +0.0 -> [(index, f)]."""
    f = np.asarray(f, dtype=np.float64) + 0.0
    ids = np.arange(f.shape[0]) if ids is None else np.unique(np.asarray(ids, dtype=np.int64))
    o = ids[np.lexsort((ids, -f[ids]))][:k]
    return [(int(i), float(f[i])) for i in o]


def canon(a):
    """The bits of an array with the sign of its zeros dropped (S19 does not promise it)."""
    return (np.ascontiguousarray(a, dtype=np.float64) + 0.0).view(np.uint64)
