"""CPU: the inputs of tests/test_gpu_diverse.py make its stepwise check an exact path check.  For that file's shapes and query
recipe, with pools from the numpy oracle's `search`: every step after the first of the reference path has a gap between the best and the
second-best margin of at least 100 tol (so within tol only the reference's pick passes), and at diversity >= 0.3 the MMR order
differs from the pool order in at least half of the cases (a no-op implementation cannot pass).  Also `diverse_ref` itself on a
hand-built pool of six rows whose path is written out by hand."""
import numpy as np
import pytest

import diverse_ref as dr
from oracle import oracle_np


def hand_pool():
    X = np.array([[1.0, 0.0, 0.0],     # 0
                  [2.0, 0.0, 0.0],     # 1: the direction of 0 (g = 1)
                  [0.0, 1.0, 0.0],     # 2: orthogonal to 0
                  [-1.0, 0.0, 0.0],    # 3: the negation of 0 (g = -1)
                  [0.0, 0.0, 0.0],     # 4: a zero row (g = 0 with everything)
                  [0.0, 3.0, 4.0]])    # 5: g = 0.6 with 2
    n64 = np.einsum("ij,ij->i", X, X)
    ids = np.arange(6)
    s = np.array([1.0, 0.9, 0.8, 0.5, 0.4, 0.7])   # (the helper does not need a sorted pool)
    return X, n64, ids, s


def test_the_reference_walks_the_hand_written_path():
    X, n64, ids, s = hand_pool()
    # delta = 0.5, m = 0.5 s - 0.5 r:
    # t = 0: r = 0                      m = .5   .45  .4   .25  .2   .35  -> 0
    # t = 1: r = g(., 0) = . 1 0 -1 0 0 m = .    -.05 .4   .75  .2   .35  -> 3 (the negation gains delta)
    # t = 2: r1 = max(1, -1) = 1        m = .    -.05 .4   .    .2   .35  -> 2
    # t = 3: r5 = g(5, 2) = .6          m = .    -.05 .    .    .2   .05  -> 4
    # t = 4:                            m = .    -.05 .    .    .    .05  -> 5, then 1
    picks, margins, gaps = dr.mmr_path(X, n64, ids, s, 6, 0.5)
    assert picks == [0, 3, 2, 4, 5, 1]
    assert margins == pytest.approx([0.5, 0.75, 0.4, 0.2, 0.05, -0.05], abs=1e-15)
    assert gaps[:5] == pytest.approx([0.05, 0.35, 0.05, 0.15, 0.10], abs=1e-15) and gaps[5] == dr.INF
    assert dr.mmr_path(X, n64, ids, s, 3, 0.5)[0] == [0, 3, 2]
    assert dr.mmr_path(X, n64, ids, s, 9, 0.5)[0] == [0, 3, 2, 4, 5, 1]
    # delta = 0: the margins are the scores; delta = 1: the scores do not count, ties go to the earlier position
    order = np.lexsort((ids, -s)).tolist()
    p0, m0, _ = dr.mmr_path(X, n64, ids, s, 6, 0.0)
    assert p0 == order and m0 == s[order].tolist()
    p1, m1, _ = dr.mmr_path(X, n64, ids, s, 6, 1.0)
    assert p1 == [0, 3, 2, 4, 5, 1] and m1 == pytest.approx([0.0, 1.0, 0.0, 0.0, -0.6, -1.0], abs=1e-15)
    # the cosines behind it
    G = dr.pool_gram(X, n64, ids)
    assert G[0, 1] == 1.0 and G[0, 3] == -1.0 and G[2, 5] == pytest.approx(0.6, abs=1e-16) and not G[4].any() and (G == G.T).all()


def test_the_stepwise_check_accepts_the_path_and_nothing_else():
    X, n64, ids, s = hand_pool()
    tol = dr.tol_for(3)
    picks, margins, _ = dr.mmr_path(X, n64, ids, s, 6, 0.5)
    good = [(int(ids[p]), float(s[p]), m) for p, m in zip(picks, margins)]
    assert dr.check_steps(good, X, n64, ids, s, 0.5, tol) == 0
    assert dr.check_steps(good[:2], X, n64, ids, s, 0.5, tol) == 0
    swapped = [good[0], good[2], good[1]] + good[3:]
    repeated = [good[0], good[0]] + good[2:]
    foreign = [good[0], (17, 0.5, 0.75)] + good[2:]
    off_margin = [good[0], (good[1][0], good[1][1], good[1][2] + 1e-9)] + good[2:]
    clamped = [good[0], (2, 0.8, 0.4)] + good[2:]   # what an implementation that clamps negative cosines picks second
    for bad in (swapped, repeated, foreign, off_margin, clamped):
        with pytest.raises(AssertionError):
            dr.check_steps(bad, X, n64, ids, s, 0.5, tol)
    # a gap below 100 tol is counted, not refused
    s2 = s.copy()
    s2[5] = s2[2] = 0.8
    X2 = X.copy()
    X2[5] = [0.0, 0.0, 1.0]
    n2 = np.einsum("ij,ij->i", X2, X2)
    picks, margins, gaps = dr.mmr_path(X2, n2, ids, s2, 6, 0.5)
    assert picks[:3] == [0, 3, 2] and gaps[2] == 0.0
    res = [(int(ids[p]), float(s2[p]), m) for p, m in zip(picks, margins)]
    assert dr.check_steps(res, X2, n2, ids, s2, 0.5, tol) == 1


@pytest.mark.parametrize("name", list(dr.SHAPES))
def test_gaps_and_reordering_on_the_gpu_tests_inputs(name):
    X, gp = dr.shape_items(name)
    n, d = X.shape
    idx = oracle_np.build(X, gp)
    n64 = np.einsum("ij,ij->i", X, X)
    tol = dr.tol_for(d)

    def served(q):
        try:
            oracle_np.search(idx, q, 0.62)
            return True
        except oracle_np.ZeroLambda:
            return False

    Q = dr.queries_of(X, np.random.default_rng(5), dr.NQ, served)
    cases = moved = 0
    cache = dr.new_cache(n)
    smallest = dr.INF
    for q in Q:
        hits, _ = oracle_np.search(idx, q, 0.62)
        ids = np.array([i for i, _ in hits])
        s = np.array([v for _, v in hits])
        P = len(ids)
        assert P == min(gp["topk"], n)
        G = dr.pool_gram(X, n64, ids, cache)
        for delta in dr.DELTAS:
            picks, _, gaps = dr.mmr_path(X, n64, ids, s, P, delta, G=G)   # (the path of a smaller n is a prefix of it)
            assert picks[0] == 0 and sorted(picks) == list(range(P))
            smallest = min([smallest] + gaps[1:])   # (step 0: r = 0, the pool's own order decides; at delta = 1 an exact tie)
            for m in sorted({min(16, P), P}):   # n = 16 and the whole pool: the first eight positions of the answer
                cases += 1
                moved += picks[:min(m, 8)] != list(range(min(m, 8)))
    print(f"{name}: smallest gap {smallest:.3g} against 100 tol = {100 * tol:.3g}; {moved} of {cases} cases reordered")
    assert smallest >= 100 * tol, (smallest, 100 * tol)
    assert 2 * moved >= cases, (moved, cases)
