"""The reference of the shortest paths over the item graph: a heap Dijkstra with plain Python float adds.  No GPU.

A graph is (n, indptr, indices, dist) as in tests/components_ref.py.  The weight of the undirected edge {u, v} is S23's: the smaller
of the dists of its stored entries, a NaN ignored (NaN if all are), -0.0 as +0.0; an edge whose weight is a NaN or negative is never
crossed.  d[v] = min over the sources s and the paths from s to v of fl(.. fl(fl(offset_s + w1) + w2) .. + wm), +inf without one."""
import heapq

import numpy as np


def weights(n, indptr, indices, dist):
    """The undirected weight of every stored entry -> float64 [nnz]."""
    indptr, cols = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    code, inv = np.unique(np.minimum(rows, cols) * n + np.maximum(rows, cols), return_inverse=True)
    w = np.full(code.shape[0], np.nan)
    np.fmin.at(w, inv, np.asarray(dist, dtype=np.float64))   # fmin ignores a NaN
    return (w + 0.0)[inv]                                    # -0.0 -> +0.0


def dijkstra(n, indptr, indices, w, ids, offsets, cutoff=None):
    """d of one source set over the entries' weights `w` (of `weights`) -> float64 [n]."""
    ip, ix, w = np.asarray(indptr), np.asarray(indices), np.asarray(w, dtype=np.float64)   # (rows become lists as they are met)
    cutoff = float("inf") if cutoff is None else float(cutoff)
    d = [float("inf")] * n
    heap = []
    for s, off in zip(ids, offsets):
        off = float(off) + 0.0
        if off <= cutoff and off < d[int(s)]:
            d[int(s)] = off
            heap.append((off, int(s)))
    heapq.heapify(heap)
    while heap:
        du, u = heapq.heappop(heap)
        if du > d[u]:
            continue
        for v, we in zip(ix[ip[u]:ip[u + 1]].tolist(), w[ip[u]:ip[u + 1]].tolist()):
            if not we >= 0.0:   # a NaN or a negative weight
                continue
            c = du + we
            if c <= cutoff and c < d[v]:
                d[v] = c
                heapq.heappush(heap, (c, v))
    return np.array(d, dtype=np.float64)


def search(n, indptr, indices, w, hits, seeds, topk, subset=None, cutoff=None):
    """The composition behind `search_geodesic`: the first `seeds` of the route's hit list [(index, score)] are the sources at
    offset 0; -> the first min(topk, |subset|) reachable items of the subset by (d, index) as [(index, d)]."""
    src = [i for i, _ in hits[:seeds]]
    d = dijkstra(n, indptr, indices, w, src, [0.0] * len(src), cutoff)
    ids = np.arange(n) if subset is None else np.asarray(subset, dtype=np.int64)
    order = ids[np.lexsort((ids, d[ids]))][:min(topk, len(ids))]
    return [(int(i), float(d[i])) for i in order if np.isfinite(d[i])]
