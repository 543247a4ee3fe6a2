"""Plain numpy reference of spherical k-means over the items: `unit` with its lane partials and halving tree, the
assignment by longdouble cosines, the update in its pinned order with the row scales as an argument, and Lloyd's loop.  Inputs
are those of kmeans_ref.py, and grid_mixture().

The error bound E = (2 d + 16) 2^-53 of a device cosine against the true one, derived with u = 2^-53 and |cos| <= 1:
  q = |c|^2 in any order: d u relative (a product and at most d - 1 adds per term); its root halves that and rounds once, the
    division rounds once: r carries (d / 2 + 2) u, every unit entry one more u;
  g = x . unit(c) in any order, fused or not: d u |x| |unit(c)|, plus u |x| |unit(c)| from the entries' own roundings and
    (d / 2 + 2) u |g| from r;
  w from the stored squared norm (d u, summed in float64): (d / 2 + 2) u; the last product: u.
Times w |x| |unit(c)| = 1 + O(d u) that is (d + 1) + (d / 2 + 2) + (d / 2 + 2) + 1 = 2 d + 6 units of u; the 10 spare units
hold every second-order term for d < 2^40.  Clamping to [-1, 1] moves a value towards the true one.  Derived, not measured."""
import numpy as np

import kmeans_ref as kr

LD = np.longdouble


def E(d):
    return (2 * d + 16) * kr.U


def grid_mixture():
    """kmeans_ref.mixture() on a grid of 2^-10: float32-exact entries, squared norms exact in any summation order."""
    return np.round(kr.mixture() * 1024) / 1024


def scales(n2):
    """w = fl(1 / fl(sqrt(n2))), NaN on a dead row: n2 of 0, NaN or inf, or a w that is not finite."""
    with np.errstate(all="ignore"):
        w = 1.0 / np.sqrt(n2)
    return np.where((n2 > 0) & np.isfinite(n2) & np.isfinite(w), w, np.nan)


def unit(v):
    """S28's unit(v) -> the unit row, or None where v has no direction."""
    p = np.zeros(-(-v.shape[0] // 64) * 64)
    p[:v.shape[0]] = v
    s = np.zeros(64)
    with np.errstate(over="ignore"):
        for trip in p.reshape(-1, 64):
            s = s + trip * trip
        for o in (32, 16, 8, 4, 2, 1):
            s[:o] = s[:o] + s[o:2 * o]
    r = scales(s[:1])[0]
    return None if np.isnan(r) else v * r


def cosines(X, C):
    """The true cosines in longdouble, from the raw rows and the raw centroids."""
    Xl, Cl = X.astype(LD), C.astype(LD)
    with np.errstate(all="ignore"):
        return (Xl @ Cl.T) / np.sqrt((Xl * Xl).sum(axis=1))[:, None] / np.sqrt((Cl * Cl).sum(axis=1))[None, :]


def assign(X, C, w):
    """-> (labels int32, cos longdouble, G): the largest cosine, ties to the smallest j; a dead row (w NaN): -1 and NaN."""
    G = cosines(X, C)
    dead = np.isnan(w) | np.isnan(G).all(axis=1)
    labels = np.where(dead, -1, np.argmax(np.where(np.isnan(G), -np.inf, G), axis=1)).astype(np.int32)
    return labels, np.where(dead, np.nan, G[np.arange(X.shape[0]), np.maximum(labels, 0)]), G


def update(X, labels, C, w):
    """y_m = fl(x_m w_m); the members of cluster j in ascending id; P_s = members [256 s, 256 s + 256) added one by one from the
    first one's y row; T = P_0 + P_1 + ..; c_j' = unit(T); an empty cluster and a T with no direction keep the centroid."""
    out = np.array(C, dtype=np.float64, copy=True)
    for j in range(C.shape[0]):
        mem = np.flatnonzero(labels == j)
        T = None
        for s in range(0, mem.size, kr.SEG):
            P = X[mem[s]] * w[mem[s]]
            for m in mem[s + 1:s + kr.SEG]:
                P = P + X[m] * w[m]
            T = P if T is None else T + P
        u = None if T is None else unit(T)
        if u is not None:
            out[j] = u
    return out


def lloyd(X, C0, w, max_iters, on_assign=None):
    """S25's loop from unit(C0) with this assign and this update -> a dict as kmeans_ref.lloyd's, with "cohesion"."""
    C, prev, changed, converged = np.stack([unit(c) for c in np.asarray(C0, dtype=np.float64)]), None, [], False
    for t in range(1, max_iters + 1):
        labels, cos, G = assign(X, C, w)
        if on_assign:
            on_assign(t, C, labels, G)
        changed.append(int(((labels >= 0) & (True if prev is None else labels != prev)).sum()))
        if changed[-1] == 0:
            converged = True
            break
        C, prev = update(X, labels, C, w), labels
    counts = np.bincount(labels[labels >= 0], minlength=C.shape[0]).astype(np.int64)
    return {"centroids": C, "labels": labels, "iterations": t, "converged": converged, "changed": changed, "counts": counts,
            "cohesion": float(cos[labels >= 0].sum()), "empty": int((counts == 0).sum())}


DEAD_ROWS = (kr.NAN_ROW, 10)


def dead_case():
    """kmeans_ref.nan_case() with one more dead row: row 10 is all zero."""
    X, C = kr.nan_case()
    X[10] = 0.0
    return X, C


def lloyd_inputs():
    """name -> (X, the starting centroids of every Lloyd run the GPU test makes on it, max_iters)."""
    out = {}
    for name, X in (("grid", grid_mixture()), ("mix", kr.mixture())):
        seed_ids = np.random.default_rng(kr.MIX_SEED).choice(X.shape[0], len(kr.MIX_INIT), replace=False)
        out[name] = (X, [X[list(kr.MIX_INIT)], X[seed_ids]], 25)
    out["dead"] = (dead_case()[0], [dead_case()[1]], 3)
    return out
