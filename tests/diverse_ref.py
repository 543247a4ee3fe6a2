"""Reference of diversified search in numpy fp64, for the tests and tools/diverse_bench.py: the greedy path over
a pool (`mmr_path`) and the stepwise check of a returned list (`check_steps`).  Item-item dots are taken pair by pair with
np.dot on 1-D rows: deterministic, so identical rows give identical cosines."""
import math

import numpy as np

INF = float("inf")


# the shapes of tests/test_gpu_diverse.py (and of the CPU check of its inputs): (n, d, k, topk, metric, kernel, rounded through float32)
SHAPES = {"1200x48": (1200, 48, 10, 64, "l2", "gaussian", False),
          "900x51": (900, 51, 8, 100, "l2", "gaussian", False),            # odd d
          "700x768f32": (700, 768, 12, 257, "l2", "gaussian", True),       # the fp32 rows widened; a pool of 4 waves x 64 + 1
          "1100x96cos": (1100, 96, 25, 1024, "cosine", "rational", False),  # the largest pool
          "300x4100": (300, 4100, 6, 20, "l2", "gaussian", False)}         # the picked row does not fit the LDS staging
DELTAS = (0.3, 0.5, 0.9, 1.0)
NQ = 6   # queries per shape


def shape_items(name):
    """(X, graph parameters) of a shape: the clustered() / calibrate_eps recipe of tests/test_gpu_range.py."""
    from conftest import calibrate_eps, clustered
    n, d, k, topk, metric, kernel, f32 = SHAPES[name]
    X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
    if f32:
        X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
    gp = {"eps": calibrate_eps(X, k, metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
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


def atol_for(d):
    """fp64 dot error of unit-norm rows (tests/test_gpu_range.py's)."""
    return 16 * d * 2.0 ** -53


def tol_for(d):
    """The cosine of two rows carries about (d + 3) 2^-53 of error and a margin at most that; two margins are compared: 64 d
    2^-53 leaves about 30 x over the worst case."""
    return 4 * atol_for(d)


def cosine(X, n64, i, j):
    """g(i, j) of S12: 0 where the product of the squared norms is not positive; not clamped."""
    den2 = n64[i] * n64[j]
    if not den2 > 0.0:
        return 0.0
    return float(np.dot(X[i], X[j])) / math.sqrt(den2)


def new_cache(nitems):
    """A cache of item-item cosines for `pool_gram` (nitems x nitems doubles: for the small indexes of the tests)."""
    return np.full((nitems, nitems), np.nan)


def pool_gram(X, n64, ids, cache=None):
    """[P, P] cosines of the pool's items, every pair once (g is symmetric), the diagonal included; pairs a cache holds are
    taken from it, the others are added to it."""
    ids = np.asarray(ids, dtype=np.int64)
    P = len(ids)
    G = np.full((P, P), np.nan) if cache is None else cache[np.ix_(ids, ids)]
    for a, b in np.argwhere(np.isnan(G)).tolist():
        if a <= b:
            G[a, b] = G[b, a] = cosine(X, n64, int(ids[a]), int(ids[b]))
    if cache is not None:
        cache[np.ix_(ids, ids)] = G
    return G


def _row(X, n64, ids, p, G):
    """The cosines of pool entry p with every entry: row p of a precomputed G, else P dots."""
    if G is not None:
        return G[p]
    return np.array([cosine(X, n64, int(ids[p]), int(j)) for j in ids])


def _margins(s, r, delta):
    with np.errstate(invalid="ignore"):
        m = (1.0 - delta) * s - delta * r
    return np.where(np.isnan(m), -INF, m)


def _update(r, g, first):
    """The largest cosine with a picked item: the first pick sets it (negative values included), later ones raise it."""
    return g.copy() if first else np.where(g > r, g, r)


def mmr_path(X, n64, ids, s, n, delta, G=None):
    """The greedy of S12 over the pool (ids, s): (positions picked, their margins, per step the gap between the best and the
    second-best margin; inf where one candidate is left).  G: the pool's cosines (`pool_gram`); without it only the rows of the
    picked entries are formed, (min(n, P) - 1) P dots."""
    ids, s = np.asarray(ids), np.asarray(s, dtype=np.float64)
    P = len(ids)
    r = np.zeros(P)
    sel = np.zeros(P, dtype=bool)
    picks, margins, gaps = [], [], []
    for t in range(min(n, P)):
        m = _margins(s, r, delta)
        cand = np.flatnonzero(~sel)
        order = cand[np.lexsort((cand, -m[cand]))]   # margin descending, position ascending
        p = int(order[0])
        picks.append(p)
        margins.append(float(m[p]))
        gaps.append(float(m[p] - m[order[1]]) if len(order) > 1 and m[p] > -INF else (INF if len(order) == 1 else 0.0))
        sel[p] = True
        if t + 1 < min(n, P):   # (the last pick needs no cosine)
            r = _update(r, _row(X, n64, ids, p, G), t == 0)
    return picks, margins, gaps


def check_steps(result, X, n64, ids, s, delta, tol, G=None):
    """The stepwise check of a returned list [(index, score, margin)] against the pool (ids, s): for every t, with r recomputed
    from the list's own prefix, the pick is an unselected pool member, its reference margin is within tol of the largest
    over the unselected, and the returned margin is within tol of the reference margin.  Returns the number of ambiguous
    steps: those whose reference gap between the best and the second-best margin is < 100 tol.  Step 0 is not counted: nothing is
    picked yet, the margins are (1 - delta) s in pool order (at delta = 1 all equal), so the tie rule decides exactly -- the
    tests require pool position 0 there."""
    ids, s = np.asarray(ids), np.asarray(s, dtype=np.float64)
    P = len(ids)
    pos = {int(i): p for p, i in enumerate(ids)}
    assert len(pos) == P, "the pool's ids are distinct"
    r = np.zeros(P)
    sel = np.zeros(P, dtype=bool)
    ambiguous = 0
    for t, (i, _, mg) in enumerate(result):
        assert i in pos, (t, i)
        p = pos[i]
        assert not sel[p], (t, i)
        m = _margins(s, r, delta)
        cand = np.sort(m[~sel])[::-1]
        best = float(cand[0])
        if best == -INF:
            assert m[p] == -INF and mg == -INF, (t, i, mg)
        else:
            assert m[p] >= best - tol, (t, i, float(m[p]), best)
            assert abs(mg - float(m[p])) <= tol, (t, i, mg, float(m[p]))
        if t > 0 and len(cand) > 1 and not (cand[0] - cand[1] >= 100 * tol):
            ambiguous += 1
        sel[p] = True
        if t + 1 < len(result):
            r = _update(r, _row(X, n64, ids, p, G), t == 0)
    return ambiguous
