"""The numpy reference of the connected components of the item graph and the hand-built inputs of its tests.  No GPU.

A graph is (n, indptr, indices, dist): the stored CSR without the diagonal, as `GraphLaplacian.to_csr_dist()` returns it.  Entry e
of row i is kept iff max_dist is None or dist[e] <= max_dist (a NaN dist is never kept under a threshold); i and j are joined iff
at least one of the stored entries i -> j, j -> i is kept; the label of an item is the smallest id of its class."""
import numpy as np

KEYS = ("count", "largest", "largest_label", "isolated", "edges_kept")   # the five numbers that do not depend on the schedule
ROUND_CAP = 64   # the GPU test's cap on the scrambled path's rounds: O(log n), against the n of a bare label propagation


def kept_entries(n, indptr, indices, dist, max_dist):
    """(rows, columns) of the kept stored entries, in CSR order."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    if max_dist is None:
        return rows, indices
    with np.errstate(invalid="ignore"):
        keep = np.asarray(dist, dtype=np.float64) <= float(max_dist)
    return rows[keep], indices[keep]


def components(n, indptr, indices, dist, max_dist=None):
    """Labels by a union-find with path halving: int32 [n], every item's label the smallest id of its class."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    rows, cols = kept_entries(n, indptr, indices, dist, max_dist)
    for i, j in zip(rows.tolist(), cols.tolist()):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)   # the smaller id stays the root: a root is its class's smallest id
    return np.array([find(x) for x in range(n)], dtype=np.int32)


def info(labels, indptr, indices, dist, max_dist=None):
    """The five schedule-free numbers of a labelling."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    sizes = np.bincount(labels, minlength=n) if n else np.zeros(0, dtype=np.int64)
    largest = int(sizes.max()) if n else 0
    return {"count": int((sizes > 0).sum()), "largest": largest, "largest_label": int(np.flatnonzero(sizes == largest)[0]) if n else 0,
            "isolated": int((sizes == 1).sum()), "edges_kept": int(kept_entries(n, indptr, indices, dist, max_dist)[0].shape[0])}


def sync_rounds(n, indptr, indices, dist, max_dist=None, parent=None):
    """The device's rounds applied synchronously -> (labels, rounds).  A round: every hook reads a = parent[i], b = parent[j] of
    the state at the round's start and proposes min(a, b) at max(a, b), the proposals of a round land as a minimum; then full
    compression.  `rounds` counts the rounds whose hook lowered something: the rounds the fixed point needs.  The device ends after
    the first round whose hook lowered nothing and counts that hook launch too: run synchronously it would report rounds + 1."""
    parent = np.arange(n, dtype=np.int64) if parent is None else np.array(parent, dtype=np.int64)
    rows, cols = kept_entries(n, indptr, indices, dist, max_dist)
    rounds = 0
    while True:
        a, b = parent[rows], parent[cols]
        ne = a != b
        if not ne.any():
            return parent.astype(np.int32), rounds
        rounds += 1
        np.minimum.at(parent, np.maximum(a, b)[ne], np.minimum(a, b)[ne])
        while True:   # full compression
            up = parent[parent]
            if (up == parent).all():
                break
            parent = up


def canonical(labels):
    """Any labelling of a partition -> the labels of S22: every class named by its smallest member."""
    labels = np.asarray(labels)
    first = np.full(int(labels.max()) + 1 if labels.size else 0, labels.shape[0], dtype=np.int64)
    np.minimum.at(first, labels, np.arange(labels.shape[0], dtype=np.int64))
    return first[labels].astype(np.int32)


# ------------------------------------------------------------------------------------------------ inputs
def csr_of_lists(n, nbrs, dists):
    """The CSR the graph stage stores for neighbour lists: entry (i, j) exists iff i lists j or j lists i, columns ascending;
    its dist is the listed pair's (the lister's own slot where both list each other).  -> (indptr, indices, dist)."""
    ent = {}
    for i in range(n):
        for j, d in zip(nbrs[i], dists[i]):
            ent.setdefault((int(i), int(j)), float(d))
    for (i, j), d in list(ent.items()):
        ent.setdefault((j, i), d)
    keys = sorted(ent)
    indptr = np.zeros(n + 1, dtype=np.int64)
    for i, _ in keys:
        indptr[i + 1] += 1
    return np.cumsum(indptr), np.array([j for _, j in keys], dtype=np.int64), np.array([ent[k] for k in keys], dtype=np.float64)


def path_lists(n, seed):
    """A path visited in a fixed random permutation of the ids, k = 2: the item at position t lists the items at positions t - 1
    and t + 1.  -> nbrs, a list of n id lists.  One component whose ids carry no order: label propagation would need n rounds."""
    perm = np.random.default_rng(seed).permutation(n)
    nbrs = [[] for _ in range(n)]
    for t in range(n):
        nbrs[int(perm[t])] = [int(perm[u]) for u in (t - 1, t + 1) if 0 <= u < n]
    return nbrs


def bridged(n_a, n_b):
    """Two rings, ids [0, n_a) and [n_a, n_a + n_b), each item listing its successor, joined by ONE pair (item 1 lists item
    n_a + 1) whose dist is strictly the largest.  -> (nbrs, dists, bridge distance): dists are made up, 1 + (i mod 7) / 16 on the
    rings (all below 1.5) and 2.0 on the bridge."""
    n = n_a + n_b
    nbrs, dists = [[] for _ in range(n)], [[] for _ in range(n)]
    for lo, m in ((0, n_a), (n_a, n_b)):
        for i in range(m):
            j = lo + (i + 1) % m
            if j != lo + i and j not in nbrs[lo + i]:
                nbrs[lo + i].append(j)
                dists[lo + i].append(1.0 + (i % 7) / 16.0)
    nbrs[1].append(n_a + 1)
    dists[1].append(2.0)
    return nbrs, dists, 2.0


MIN_GAP = 1e-6   # every threshold placed by gap_thresholds sits in a relative gap of at least this between distinct stored distances


def distinct_distances(dist):
    d = np.asarray(dist, dtype=np.float64)
    return np.unique(d[np.isfinite(d)])


def gap_thresholds(dist, count):
    """`count` thresholds across the range of the stored distances, each the midpoint of a gap between neighbouring distinct
    values whose relative width is at least MIN_GAP: near the quantiles (j + 1) / (count + 1), the nearest such gap at or above."""
    u = distinct_distances(dist)
    assert u.shape[0] >= 2
    wide = np.flatnonzero((u[1:] - u[:-1]) >= MIN_GAP * np.abs(u[1:]))
    assert wide.shape[0] >= 1
    out = []
    for j in range(count):
        at = int(round((j + 1) * (u.shape[0] - 1) / (count + 1)))
        g = wide[min(np.searchsorted(wide, min(at, u.shape[0] - 2)), wide.shape[0] - 1)]
        out.append(0.5 * (u[g] + u[g + 1]))
    return out


def gap_of(dist, t):
    """The relative distance from t to the nearest distinct stored distance (inf without one)."""
    u = distinct_distances(dist)
    return float(np.min(np.abs(u - t) / np.maximum(np.abs(u), 1e-300))) if u.shape[0] else float("inf")
