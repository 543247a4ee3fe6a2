"""Plain numpy reference of k-means over the items: distances by direct differences in float64, the derived error
bound of the device's keys, the update in its pinned summation order and Lloyd's loop.  Also the inputs the GPU tests and their
CPU companions share."""
import numpy as np

SEG = 256          # members of an update segment: part of S25's definition
U = 2.0 ** -53


def dists(X, C):
    """D[i, j] = sum_c (x_ic - c_jc)^2, every difference formed directly."""
    return np.stack([((X - c) ** 2).sum(axis=1) for c in C], axis=1)


def bound(X, C):
    """E[i, j] = (2 d + 8) 2^-53 (|x_i|^2 + |c_j|^2): any summation order of a length-d float64 dot, of the two norms, and the three
    roundings of key and dist stay inside it (fused products only tighten it).  Derived, not measured."""
    d = X.shape[1]
    return (2 * d + 8) * U * ((X * X).sum(axis=1)[:, None] + (C * C).sum(axis=1)[None, :])


def assign(X, C):
    """-> (labels int32, dist, D): the nearest centroid, ties to the smallest j; a row without a comparable distance: -1 and NaN."""
    D = dists(X, C)
    dead = np.isnan(D).all(axis=1)
    labels = np.where(dead, -1, np.argmin(np.where(np.isnan(D), np.inf, D), axis=1)).astype(np.int32)
    dist = np.where(dead, np.nan, D[np.arange(X.shape[0]), np.maximum(labels, 0)])
    return labels, dist, D


def update(X, labels, C):
    """The members of cluster j in ascending id; P_s = members [256 s, 256 s + 256) added one by one from the first one's row;
    T = P_0 + P_1 + ..; c_j' = T / count; an empty cluster keeps its centroid."""
    out = np.array(C, dtype=np.float64, copy=True)
    for j in range(C.shape[0]):
        mem = np.flatnonzero(labels == j)
        if not mem.size:
            continue
        T = None
        for s in range(0, mem.size, SEG):
            P = X[mem[s]].copy()
            for m in mem[s + 1:s + SEG]:
                P = P + X[m]
            T = P if T is None else T + P
        out[j] = T / float(mem.size)
    return out


def lloyd(X, C0, max_iters, on_assign=None):
    """Lloyd's loop of S25 -> dict(centroids, labels, iterations, converged, changed, counts, inertia, empty)."""
    C, prev, changed, converged = np.array(C0, dtype=np.float64), None, [], False
    for t in range(1, max_iters + 1):
        labels, dist, D = assign(X, C)
        if on_assign:
            on_assign(t, C, labels, D)
        changed.append(int(((labels >= 0) & (True if prev is None else labels != prev)).sum()))
        if changed[-1] == 0:
            converged = True
            break
        C, prev = update(X, labels, C), labels
    counts = np.bincount(labels[labels >= 0], minlength=C.shape[0]).astype(np.int64)
    return {"centroids": C, "labels": labels, "iterations": t, "converged": converged, "changed": changed, "counts": counts,
            "inertia": float(dist[labels >= 0].sum()), "dist": dist, "empty": int((counts == 0).sum())}


# ---- inputs
MIX = (1283, 33, 6)   # the Lloyd runs and the update's bits: n = 0 + 1 + 255 + 256 + 257 + 513 members and one item without a label
SIZES = (0, 1, 255, 256, 257, 513)
MIX_INIT, MIX_SEED, NAN_ROW = (3, 700, 41, 1200, 515, 88), 11, 64


def mixture(f32=False):
    """A well-separated mixture of MIX[2] clusters, unnormalised; f32: rounded through float32 (the fp32-row path)."""
    from conftest import clustered
    n, d, nclust = MIX
    X = 4.0 * clustered(n, d, nclust=nclust, noise=0.08, seed=77, normalise=False)
    return np.ascontiguousarray(X.astype(np.float32).astype(np.float64)) if f32 else X


def interleaved_labels():
    """Labels with the cluster sizes SIZES interleaved in id, and -1 on the last item."""
    lab = np.concatenate([np.full(c, j) for j, c in enumerate(SIZES)])
    lab = np.random.default_rng(5).permutation(lab)
    return np.concatenate([lab, [-1]]).astype(np.int32)


def integer_items(n, d, seed):
    """Integer-valued items in [-8, 8]: every product with a multiple of 0.5 and every partial sum is exact in any order."""
    return np.random.default_rng(seed).integers(-8, 9, (n, d)).astype(np.float64)


def half_centroids(X, k, seed):
    """k centroids that are multiples of 0.5; 0 and 1 identical; item 5 at 0.25 from centroids 2 and 3 alike (k >= 4)."""
    C = np.random.default_rng(seed).integers(-16, 17, (k, X.shape[1])) * 0.5
    if k >= 2:
        C[1] = C[0]
    if k >= 4:
        C[2], C[3] = X[5], X[5]
        C[2, 0] += 0.5
        C[3, 0] -= 0.5
    return C


def gaussian_items(n, d, seed):
    from conftest import clustered
    return clustered(n, d, nclust=5, noise=0.3, seed=seed) * (1 + 1e-9)


def nan_case():
    """129 x 33 fp64 items whose row NAN_ROW holds one NaN, and three centroids drawn from the other rows."""
    X = gaussian_items(129, 33, 129 + 33)
    X[NAN_ROW, 7] = np.nan
    return X, jittered_centroids(np.delete(X, NAN_ROW, axis=0), 3, 9)


def jittered_centroids(X, k, seed):
    rng = np.random.default_rng(seed)
    return X[rng.integers(0, X.shape[0], k)] + 0.01 * rng.standard_normal((k, X.shape[1]))
