"""GPU: ArrowSpace.search_batch_taus -- B queries under several taus, the distinct taus in [0, 1] sharing the batched passes
of search_batch (one scan, k-NN step and lambda_q per 32 queries, a scorer tail per (query, tau) pair).  Entry [b][j] must
be exactly (list equality) search(Q[b], gl, taus[j]); the shared tail must really run; whatever it does not serve must
come back from the single search."""
import os
import sys
import threading

import numpy as np
import pytest

from conftest import assert_hits_match, calibrate_eps, clustered, gpu_clustered
from test_gpu_parity import RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TAU_SETS = [[1.0, 0.8, 0.62], [0.62, 0.8, 0.42, 0.0], [0.0, 0.0], [0.62, 0.62, 0.3], [float(t) for t in np.linspace(0.0, 1.0, 11)]]


def queries(X, nq, seed, scale=0.05):
    rng = np.random.default_rng(seed)
    n, d = X.shape
    return np.ascontiguousarray(X[rng.integers(0, n, nq)] + scale * rng.standard_normal((nq, d)) / np.sqrt(d))


def check_equal(aspace, gl, Q, taus, got, rows=None):
    assert len(got) == Q.shape[0]
    for b in (range(Q.shape[0]) if rows is None else rows):
        assert len(got[b]) == len(taus)
        for j, tau in enumerate(taus):
            assert got[b][j] == aspace.search(Q[b], gl, tau), (b, tau)


def in_range_distinct(taus):
    return len({np.float64(t).tobytes() for t in taus if 0.0 <= t <= 1.0})


@pytest.mark.parametrize("n,d,k,topk,metric,kernel", [(1200, 48, 10, 10, "l2", "gaussian"), (3000, 96, 25, 10, "cosine", "rational"),
                                                       (2000, 768, 25, 15, "l2", "gaussian"), (20000, 384, 4, 2, "l2", "gaussian"),
                                                       (1500, 1000, 10, 8, "l2", "gaussian")])
def test_batch_sweep_equals_single_search(oracle_lib, n, d, k, topk, metric, kernel):
    import pyarrowspace_amd as asp
    X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
    gp = {"eps": calibrate_eps(X, k, metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    ref = oracle_lib.OracleIndex(X, gp)
    Qall = queries(X, 100, seed=n)
    for bi, B in enumerate((2, 31, 32, 33, 100)):
        Q = np.ascontiguousarray(Qall[:B])
        taus = TAU_SETS[bi % len(TAU_SETS)]
        c0 = aspace.batch_sweep_counters()
        got = aspace.search_batch_taus(Q, gl, taus)
        c1 = aspace.batch_sweep_counters()
        assert c1["calls"] == c0["calls"] + 1
        rows = range(B) if B <= 33 else range(0, B, 7)
        check_equal(aspace, gl, Q, taus, got, rows)
        for j, tau in enumerate(taus):
            assert [got[b][j] for b in range(B)] == aspace.search_batch(Q, gl, tau)
        for b in list(rows)[:2]:
            for tau in taus[:2]:
                j = taus.index(tau)
                want, lq_ref = ref.search(Q[b], tau)
                assert_hits_match(got[b][j], want, ref.scores(Q[b], tau, lq_ref), rtol=RTOL)


def test_shared_tail_runs_and_serves_every_pair():
    import pyarrowspace_amd as asp
    X = clustered(6000, 128, nclust=64, seed=3)
    gp = {"eps": calibrate_eps(X, 10), "k": 10, "topk": 10, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    Q = queries(X, 70, seed=8)
    for taus in TAU_SETS:
        c0 = aspace.batch_sweep_counters()
        got = aspace.search_batch_taus(Q, gl, taus)
        c1 = aspace.batch_sweep_counters()
        assert c1["shared_passes"] > c0["shared_passes"], (c0, c1)
        if c1["pairs_redone"] == c0["pairs_redone"]:
            assert c1["pairs_served"] - c0["pairs_served"] == len(Q) * in_range_distinct(taus), (taus, c0, c1)
        check_equal(aspace, gl, Q, taus, got, range(0, len(Q), 5))


def test_edge_taus_and_empty_inputs():
    import pyarrowspace_amd as asp
    X = clustered(1500, 64, nclust=12, seed=2)
    gp = {"eps": calibrate_eps(X, 8), "k": 8, "topk": 6, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    Q = queries(X, 40, seed=1, scale=0.02)
    taus = [1.0, -0.5, 0.62, 1.5, 0.62, 0.0]
    check_equal(aspace, gl, Q, taus, aspace.search_batch_taus(Q, gl, taus))
    try:
        want = [aspace.search(Q[b], gl, float("nan")) for b in range(len(Q))]
    except Exception as e:   # noqa: BLE001
        with pytest.raises(type(e)):
            aspace.search_batch_taus(Q, gl, [float("nan"), 0.8])
    else:
        got = aspace.search_batch_taus(Q, gl, [float("nan"), 0.8])
        assert [g[0] for g in got] == want
        check_equal(aspace, gl, Q, [0.8], [[g[1]] for g in got])
    assert aspace.search_batch_taus(Q, gl, []) == [[] for _ in range(len(Q))]
    assert aspace.search_batch_taus(np.zeros((0, 64)), gl, [1.0, 0.5]) == []
    one = np.ascontiguousarray(Q[:1])
    check_equal(aspace, gl, one, [1.0, 0.62], aspace.search_batch_taus(one, gl, [1.0, 0.62]))
    with pytest.raises(ValueError, match="query length"):
        aspace.search_batch_taus(np.ascontiguousarray(Q[:, :10]), gl, [1.0, 0.8])


def test_zero_lambda_panics_as_search_batch_does():
    import pyarrowspace_amd as asp
    X = clustered(800, 32, nclust=8, seed=4)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    Q = queries(X, 5, seed=2, scale=0.01)
    Q[3] = 50.0   # no item within eps: lambda_q == 0
    with pytest.raises(asp.PanicException):
        aspace.search_batch(Q, gl, 0.62)
    with pytest.raises(asp.PanicException):
        aspace.search_batch_taus(Q, gl, [1.0, 0.62, 0.0])


def test_overflowing_pairs_fall_back_exactly():
    """mass duplicates (6 points x 400 copies): ties past a candidate buffer; the pairs a shared pass cannot prove are redone
    and the answers stay the single searches'."""
    import pyarrowspace_amd as asp
    rng = np.random.default_rng(0)
    base = rng.standard_normal((6, 16))
    X = np.repeat(base, 1000, axis=0) + 1e-9 * rng.standard_normal((6000, 16))
    gp = {"eps": 0.5, "k": 5, "topk": 6, "p": 2.0, "sigma": 0.3}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    Q = np.ascontiguousarray(np.repeat(base, 6, axis=0)[:34] * 1.001)
    taus = [1.0, 0.62, 0.3, 0.0]
    c0 = aspace.batch_sweep_counters()
    got = aspace.search_batch_taus(Q, gl, taus)
    c1 = aspace.batch_sweep_counters()
    check_equal(aspace, gl, Q, taus, got)
    assert c1["pairs_redone"] > c0["pairs_redone"], (c0, c1)


def test_crowded_neighbourhood_and_feature_mode():
    import arrowspace
    X = clustered(5000, 64, nclust=6, noise=0.4, seed=23, normalise=False) * 100.0
    gp = {"eps": 10.0, "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = arrowspace.ArrowSpaceBuilder.build(gp, X)
    Q = np.ascontiguousarray(X[np.random.default_rng(9).integers(0, 5000, 40)] * 1.02)
    taus = [1.0, 0.8, 0.62, 0.0]
    check_equal(aspace, gl, Q, taus, aspace.search_batch_taus(Q, gl, taus), range(0, 40, 3))
    from conftest import calibrate_feature_eps
    Xf = clustered(1500, 96, nclust=12, seed=11)
    gpf = {"eps": calibrate_feature_eps(Xf, 6), "k": 6, "topk": 8, "p": 2.0, "sigma": None, "lambda_mode": "feature", "metric": "cosine",
           "kernel": "rational"}
    import pyarrowspace_amd as asp
    fs, fgl = asp.ArrowSpaceBuilder.build(gpf, Xf)
    Qf = queries(Xf, 35, seed=4, scale=0.02)
    check_equal(fs, fgl, Qf, [1.0, 0.62, 0.0], fs.search_batch_taus(Qf, fgl, [1.0, 0.62, 0.0]), range(0, 35, 4))


def test_batch_sweep_beside_concurrent_searches():
    import pyarrowspace_amd as asp
    X = clustered(30000, 128, nclust=64, seed=31)
    gp = {"eps": calibrate_eps(X, 10), "k": 10, "topk": 10, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    Q = queries(X, 40, seed=12)
    taus = [1.0, 0.8, 0.62, 0.0]
    serial_sweep = aspace.search_batch_taus(Q, gl, taus)
    serial_batch = aspace.search_batch(Q, gl, 0.62)
    serial = [[aspace.search(Q[b], gl, t) for t in taus] for b in range(6)]
    assert [s[2] for s in serial_sweep] == serial_batch
    errors = []

    def run(fn):
        try:
            for _ in range(4):
                fn()
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    def sweeper():
        assert aspace.search_batch_taus(Q, gl, taus) == serial_sweep

    def batcher():
        assert aspace.search_batch(Q, gl, 0.62) == serial_batch

    def single():
        for b in range(6):
            for j, t in enumerate(taus):
                assert aspace.search(Q[b], gl, t) == serial[b][j]

    th = [threading.Thread(target=run, args=(f,)) for f in (sweeper, batcher, single, single)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]


def test_headline_size_batch_sweep_equals_search_batch():
    import pyarrowspace_amd as asp
    import bench
    import torch
    n, d, k, topk = 1_000_000, 768, 25, 15
    X = gpu_clustered(n, d, 42)
    gp = {"eps": bench.calibrate_eps(X, k, "l2"), "k": k, "topk": topk, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    rng = np.random.default_rng(21)
    rows = torch.as_tensor(rng.integers(0, n, 256), device=X.device)
    Q = np.ascontiguousarray(X[rows].cpu().double().numpy() + 0.05 * rng.standard_normal((256, d)) / np.sqrt(d))
    del X
    taus = [1.0, 0.8, 0.62]
    c0 = aspace.batch_sweep_counters()
    got = aspace.search_batch_taus(Q, gl, taus)
    c1 = aspace.batch_sweep_counters()
    assert c1["shared_passes"] > c0["shared_passes"], (c0, c1)
    for j, tau in enumerate(taus):
        assert [g[j] for g in got] == aspace.search_batch(Q, gl, tau), tau
    for b in range(0, 256, 64):
        for j, tau in enumerate(taus):
            assert got[b][j] == aspace.search(Q[b], gl, tau)
