"""Mode must not leak from one search entry point into the next: every single-query call of one thread is served by the
same pooled workspace, and the batched calls share theirs, so whatever a driver leaves behind on a workspace (fused tail,
coarse scan, coarse chain, crowded hints, tau of the last scan) is what the next entry point starts from."""
import numpy as np
import pytest

from conftest import assert_hits_match, calibrate_eps, clustered

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def test_entry_points_in_either_order_return_the_same_hits(oracle_lib):
    """The index of test_coarse_scan_returns_what_the_two_digit_scan_returns (it reaches the fused tail, the coarse scan and
    the coarse chain), six kinds of call forwards and then backwards on the same ArrowSpace: every result matches the
    oracle, every call returns the same hits (==) in both runs, and no search needed a rerun."""
    import pyarrowspace_amd as asp
    n, d, k, topk = 30000, 256, 12, 9
    X = clustered(n, d, nclust=150, seed=71)
    gp = {"eps": calibrate_eps(X, k, "l2"), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": "l2"}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    ref = oracle_lib.OracleIndex(X, gp)
    rng = np.random.default_rng(11)
    QB = np.ascontiguousarray(X[rng.integers(0, n, 40)] + 0.03 * rng.standard_normal((40, d)) / np.sqrt(d))   # a pair of passes: 32 + 8
    Q1 = [np.ascontiguousarray(q) for q in QB[:8]]

    oracle = {}

    def check(got, q, tau):
        key = (q.tobytes(), tau)
        if key not in oracle:
            want, lq = ref.search(q, tau)
            oracle[key] = (want, ref.scores(q, tau, lq))
        assert_hits_match(got, *oracle[key], rtol=RTOL)

    def single(tau):
        out = [aspace.search(q, gl, tau) for q in Q1]
        for q, got in zip(Q1, out):
            check(got, q, tau)
        return out

    def taus_single(taus):
        out = [aspace.search_taus(q, gl, taus) for q in Q1]
        for q, lists in zip(Q1, out):
            assert len(lists) == len(taus)
            for tau, got in zip(taus, lists):
                check(got, q, tau)
        return out

    def batch(tau):
        out = aspace.search_batch(QB, gl, tau)
        assert len(out) == len(QB)
        for q, got in zip(QB, out):
            check(got, q, tau)
        return out

    def taus_batch(taus):
        out = aspace.search_batch_taus(QB, gl, taus)
        assert len(out) == len(QB)
        for q, lists in zip(QB, out):
            assert len(lists) == len(taus)
            for tau, got in zip(taus, lists):
                check(got, q, tau)
        return out

    calls = [lambda: single(0.62), lambda: single(0.2), lambda: taus_single([0.2, 0.5, 0.9]), lambda: batch(0.62),
             lambda: taus_batch([0.3, 0.8]), lambda: single(1.0)]
    forward = [c() for c in calls]
    backward = [c() for c in reversed(calls)][::-1]
    for i, (f, b) in enumerate(zip(forward, backward)):
        assert f == b, i
    assert aspace.search_counters()["searches_with_rerun"] == 0
