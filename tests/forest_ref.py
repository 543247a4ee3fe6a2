"""The numpy reference of the minimum spanning forest of the item graph and the hand-built inputs of its tests.  No GPU.

A graph is (n, indptr, indices, dist) as in tests/components_ref.py.  The weight of the undirected edge {u < v} is the smaller of
the dists of its stored entries, a NaN ignored (NaN if all are; a zero is +0.0); edges are ordered by (w ascending with NaN after
+inf, then u, then v), and the forest is Kruskal's under that order."""
import numpy as np

MONOTONE_N = 4099


def edges(n, indptr, indices, dist):
    """The distinct undirected edges in the total order -> (u, v, w)."""
    indptr, cols = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    code, inv = np.unique(np.minimum(rows, cols) * n + np.maximum(rows, cols), return_inverse=True)
    w = np.full(code.shape[0], np.nan)
    np.fmin.at(w, inv, np.asarray(dist, dtype=np.float64))   # fmin ignores a NaN
    w = w + 0.0                                              # -0.0 -> +0.0
    u, v = code // max(n, 1), code % max(n, 1)
    order = np.lexsort((v, u, np.where(np.isnan(w), np.inf, w), np.isnan(w)))
    return u[order].astype(np.int32), v[order].astype(np.int32), w[order]


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def kruskal(n, indptr, indices, dist):
    """The minimum spanning forest in the total order -> (u, v, w)."""
    u, v, w = edges(n, indptr, indices, dist)
    parent, keep = list(range(n)), []
    for e, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            keep.append(e)
    return u[keep], v[keep], w[keep]


def cut(n, u, v, w, t):
    """The labels of S22 from the forest's edges with w <= t (None: all): every item named by the smallest id of its class."""
    parent = list(range(n))
    with np.errstate(invalid="ignore"):
        keep = np.ones(len(w), dtype=bool) if t is None else np.asarray(w) <= t
    for a, b in zip(np.asarray(u)[keep].tolist(), np.asarray(v)[keep].tolist()):
        ra, rb = _find(parent, a), _find(parent, b)
        parent[max(ra, rb)] = min(ra, rb)   # the smaller id stays the root
    return np.array([_find(parent, x) for x in range(n)], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ inputs
def twoway(n=65):
    """A ring in which i and i + 1 both list each other with made-up, different dists (forward 1 + (i mod 5) / 8, backward
    1.03125 + (3 i mod 7) / 16: the two sets share no value); the pair (7, 8) has a NaN forward and a number backward.
    -> (nbrs, dists)."""
    nbrs, dists = [], []
    for i in range(n):
        nbrs.append([(i + 1) % n, (i - 1) % n])
        dists.append([float("nan") if i == 7 else 1.0 + (i % 5) / 8.0, 1.03125 + ((3 * ((i - 1) % n)) % 7) / 16.0])
    return nbrs, dists


def monotone(n=MONOTONE_N):
    """The path in id order, item i listing i + 1 at the strictly increasing dist 1 + i / 8192: in the first round every item but
    0 picks its edge to the smaller id, and 0 and 1 pick each other: one chain of n - 1 hooks.  -> (nbrs, dists)."""
    return [[i + 1] if i + 1 < n else [] for i in range(n)], [[1.0 + i / 8192.0] if i + 1 < n else [] for i in range(n)]
