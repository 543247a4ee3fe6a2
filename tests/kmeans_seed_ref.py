"""Plain numpy restatement of the greedy k-means++ seeding: the distance in the device's arithmetic, the potential
in its pinned order (segments of 256 rows, the halving tree, ascending prefixes), the sampling walk, the greedy step and the fill
rule; and the exact replay that bounds a run on real-valued items.  Inputs come from tests/kmeans_ref.py."""
import math

import numpy as np

import kmeans_ref as kr

SEG = 256


def default_trials(k):
    return min(16, 2 + int(math.floor(math.log(k))))


def draws(n, k, L, seed):
    rng = np.random.default_rng(seed)
    return int(rng.integers(n)), rng.random((k - 1, L))


def fold(m, X, n64, c):
    """min(m, d(., c)), d = max(0, fl(n64 + fl(n64[c] - fl(2 dot)))); a NaN d -> weight 0; the candidate's own weight +0.0."""
    with np.errstate(invalid="ignore"):
        dd = n64 + (n64[c] - 2.0 * (X @ X[c]))
    g = np.where(np.isnan(dd), 0.0, np.minimum(m, np.nan_to_num(np.where(dd < 0.0, 0.0, dd), nan=0.0)))
    g[c] = 0.0
    return g


def potential(m):
    """-> (P, T): the segment sums by the halving tree and their ascending prefixes; Phi = T[-1]."""
    S = (m.shape[0] + SEG - 1) // SEG
    v = np.zeros((S, SEG))
    v.reshape(-1)[:m.shape[0]] = m
    o = SEG // 2
    while o:
        v[:, :o] = v[:, :o] + v[:, o:2 * o]
        o //= 2
    P, T, run = v[:, 0].copy(), np.empty(S), 0.0
    for s in range(S):
        run = run + P[s]
        T[s] = run
    return P, T


def sample(m, P, T, u):
    t = u * T[-1]
    above = np.flatnonzero(T > t)
    s = int(above[0]) if above.size else int(np.flatnonzero(P > 0)[-1])
    r, last = (T[s - 1] if s else 0.0), -1
    for j in range(s * SEG, min((s + 1) * SEG, m.shape[0])):
        r = r + m[j]
        if m[j] > 0:
            last = j
            if r > t:
                return j
    return last


def seed(X, k, L, seed):
    """S26 -> dict(ids, phi, candidates, chosen, degenerate)."""
    n, n64 = X.shape[0], (X * X).sum(axis=1)
    first, U = draws(n, k, L, seed)
    m = fold(np.full(n, np.inf), X, n64, first)
    P, T = potential(m)
    ids, phi = [first], [T[-1]]
    cands, chosen, degenerate = np.full((k - 1, L), -1, dtype=np.int64), np.full(k - 1, -1, dtype=np.int32), 0
    for t in range(1, k):
        if not phi[-1] > 0:
            ids.append(min(set(range(n)) - set(ids)))
            phi.append(0.0)
            degenerate += 1
            continue
        best = None
        for l in range(L):
            c = sample(m, P, T, U[t - 1, l])
            cands[t - 1, l] = c
            ml = fold(m, X, n64, c)
            Pl, Tl = potential(ml)
            if best is None or Tl[-1] < best[0]:
                best = (Tl[-1], l, c, ml, Pl, Tl)
        chosen[t - 1], m, P, T = best[1], *best[3:]
        ids.append(best[2])
        phi.append(best[0])
    return {"ids": np.array(ids, dtype=np.int64), "phi": np.array(phi), "candidates": cands, "chosen": chosen, "degenerate": degenerate}


def repeated_items():
    """257 integer rows that repeat 5 distinct ones: with k = 7 the last two picks are the fill rule's."""
    return kr.integer_items(5, 33, 5)[np.random.default_rng(6).integers(0, 5, 257)]


def check_replay(X, k, L, seed, ids, info, live=None):
    """A run on real-valued items against exact distances (`kr.dists`).  delta = sum_i max_j E[i, j] (`kr.bound`, j over every row
    the run touched) bounds the sum of |m - exact m|; n 2^-53 Phi the summation and the rounding of u Phi.  `live`: the rows that
    count (a row with a NaN is in no potential)."""
    n, live = X.shape[0], np.ones(X.shape[0], dtype=bool) if live is None else live
    first, U = draws(n, k, L, seed)
    phi, cands, chosen = info["phi"], info["candidates"], info["chosen"]
    assert ids[0] == first and len(set(ids.tolist())) == k and ids.min() >= 0 and ids.max() < n and live[ids].all()
    assert info["degenerate"] == 0 and (cands >= 0).all() and (cands < n).all() and live[cands].all()
    assert np.array_equal(ids[1:], cands[np.arange(k - 1), chosen])
    touched = np.unique(np.concatenate([ids, cands.reshape(-1)]))
    Xl = np.where(live[:, None], X, 0.0)
    D = dict(zip(touched.tolist(), np.where(live[:, None], kr.dists(Xl, Xl[touched]), 0.0).T))
    delta = kr.bound(Xl, Xl[touched]).max(axis=1)[live].sum()
    m, worst = D[first].copy(), 0.0
    for t in range(k):
        if t:
            cum, slack = np.cumsum(m), delta + n * kr.U * m.sum()
            for l in range(L):
                c, tt = int(cands[t - 1, l]), U[t - 1, l] * phi[t - 1]
                assert cum[c] - m[c] - slack <= tt <= cum[c] + slack, (t, l)
            pots = [np.minimum(m, D[int(c)]).sum() for c in cands[t - 1]]
            assert pots[chosen[t - 1]] <= min(pots) + 2.0 * slack, t
            m = np.minimum(m, D[int(ids[t])])
        slack = delta + n * kr.U * m.sum()
        worst = max(worst, abs(phi[t] - m.sum()) / slack)
        assert abs(phi[t] - m.sum()) <= slack, t
    print(f"phi: {worst:.3g} of its bound at most")
