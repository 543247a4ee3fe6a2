"""GPU: ArrowSpace.search_taus -- one query under several taus, served by shared passes over the items (one coarse scan,
one k-NN step, one exact evaluation of the union of the taus' candidates, one ranking per tau).  List j must be what
`search(item, gl, taus[j])` returns and what the oracle returns for taus[j]; the shared pass must really run where the
coarse chain can take the workspace; whatever it does not serve must come back from the single search."""
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

TAU_SETS = [[1.0, 0.8, 0.62], [0.62, 0.8, 0.42, 0.0], [0.0, 0.0], [0.62, 0.62, 0.3], list(np.linspace(0.0, 1.0, 11))]


def same_as_single(sweep, single, tie=1e-12):
    """The sweep's list against search()'s: the same indices in the same order except where two scores tie to `tie`
    relative, scores within `tie` relative."""
    assert len(sweep) == len(single), (sweep, single)
    gs = np.array([s for _, s in sweep])
    ws = np.array([s for _, s in single])
    np.testing.assert_allclose(gs, ws, rtol=tie, atol=0.0)
    for t, ((a, _), (b, _)) in enumerate(zip(sweep, single)):
        if a != b:
            tied = [u for u in range(len(ws)) if abs(ws[u] - ws[t]) <= tie * max(abs(ws[t]), 1e-300)]
            assert len(tied) > 1 and a in [single[u][0] for u in tied], (t, sweep, single)


def check_sweep(aspace, gl, q, taus, ref=None):
    got = aspace.search_taus(q, gl, taus)
    assert len(got) == len(taus)
    lq = aspace.query_lambda(q, gl)
    for j, tau in enumerate(taus):
        same_as_single(got[j], aspace.search(q, gl, tau))
        if ref is not None:
            want, lq_ref = ref.search(q, tau)
            assert_hits_match(got[j], want, ref.scores(q, tau, lq_ref), rtol=RTOL)
            assert abs(lq - lq_ref) <= RTOL * abs(lq_ref)
    return got


@pytest.mark.parametrize("n,d,k,topk,metric,kernel", [(1200, 48, 10, 10, "l2", "gaussian"), (3000, 96, 25, 10, "cosine", "rational"),
                                                       (2000, 768, 25, 15, "l2", "gaussian"), (20000, 384, 4, 2, "l2", "gaussian")])
def test_sweep_matches_oracle_and_single_search(oracle_lib, n, d, k, topk, metric, kernel):
    import pyarrowspace_amd as asp
    X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
    gp = {"eps": calibrate_eps(X, k, metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    ref = oracle_lib.OracleIndex(X, gp)
    rng = np.random.default_rng(5)
    for _ in range(3 if n < 10000 else 2):
        q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        try:
            ref.search(q, 1.0)
        except oracle_lib.ZeroLambda:
            continue
        for taus in TAU_SETS:
            check_sweep(aspace, gl, q, taus, ref)
    assert aspace.search_taus(np.ascontiguousarray(X[0]), gl, []) == []


def test_sweep_outputs_lambda_q_and_edge_taus():
    """out_lambda_q is query_lambda; taus outside [0, 1] and NaN are whatever search() returns for them."""
    import pyarrowspace_amd as asp
    X = clustered(1500, 64, nclust=12, seed=2)
    gp = {"eps": calibrate_eps(X, 8), "k": 8, "topk": 6, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    q = np.ascontiguousarray(X[17] * 1.01)
    lq = sweep_lambda_q(aspace, gl, q, [1.0, 0.5])
    assert lq == aspace.query_lambda(q, gl)
    taus = [1.0, -0.5, 0.62, 1.5, 0.62]
    got = aspace.search_taus(q, gl, taus)
    for j, tau in enumerate(taus):
        same_as_single(got[j], aspace.search(q, gl, tau))
    try:
        want = aspace.search(q, gl, float("nan"))
    except Exception as e:   # noqa: BLE001
        with pytest.raises(type(e)):
            aspace.search_taus(q, gl, [float("nan"), 0.8])
    else:
        got = aspace.search_taus(q, gl, [float("nan"), 0.8])
        assert [i for i, _ in got[0]] == [i for i, _ in want]
        same_as_single(got[1], aspace.search(q, gl, 0.8))
    with pytest.raises(TypeError):
        aspace.search_taus(q.astype(np.float32), gl, [1.0, 0.8])
    with pytest.raises(ValueError, match="query length"):
        aspace.search_taus(np.ascontiguousarray(q[:10]), gl, [1.0, 0.8])


def sweep_lambda_q(aspace, gl, q, taus):
    import ctypes as C

    import pyarrowspace_amd as asp
    t = np.asarray(taus, dtype=np.float64)
    topk = min(gl.graph_params["topk"], aspace.nitems)
    idx = np.empty((len(t), topk), dtype=np.int64)
    sc = np.empty((len(t), topk), dtype=np.float64)
    ln = np.zeros(len(t), dtype=np.int64)
    lq = C.c_double(-1.0)
    st = asp._L.as_search_taus(aspace._h, gl._h, q.ctypes.data, q.shape[0], t.ctypes.data, len(t), idx.ctypes.data, sc.ctypes.data,
                               ln.ctypes.data, C.byref(lq))
    assert st == 0
    return lq.value


def torch_rows(X, rows):
    import torch
    return torch.as_tensor(np.asarray(rows), device=X.device)


def test_shared_pass_runs_once_per_call_at_200k():
    import pyarrowspace_amd as asp
    import bench
    n, d, k, topk = 200_000, 768, 25, 15
    X = gpu_clustered(n, d, 42)
    gp = {"eps": bench.calibrate_eps(X, k, "l2"), "k": k, "topk": topk, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    rng = np.random.default_rng(3)
    Xq = X[torch_rows(X, rng.integers(0, n, 32))].cpu().double().numpy()
    del X
    taus = [1.0, 0.8, 0.62]
    for i in range(32):
        q = np.ascontiguousarray(Xq[i] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        c0 = aspace.sweep_counters()
        got = aspace.search_taus(q, gl, taus)
        c1 = aspace.sweep_counters()
        assert c1["calls"] == c0["calls"] + 1
        assert c1["shared_passes"] == c0["shared_passes"] + 1, (i, c0, c1)
        assert c1["taus_redone"] == c0["taus_redone"] == 0, (i, c0, c1)
        assert aspace.last_scan_operand == "int8-high"
        if i % 4 == 0:
            for j, tau in enumerate(taus):
                same_as_single(got[j], aspace.search(q, gl, tau))


@pytest.mark.parametrize("extra", [{"force_exact": True}, {"_search_mode": 1}, {"_search_mode": 2}, {"_search_mode": 3},
                                   {"lambda_mode": "feature", "metric": "cosine", "kernel": "rational"}])
def test_workspaces_the_chain_cannot_take_fall_back_to_single_searches(extra):
    import pyarrowspace_amd as asp
    n, d = 1500, 96
    X = clustered(n, d, nclust=12, seed=11)
    if extra.get("lambda_mode") == "feature":
        from conftest import calibrate_feature_eps
        eps = calibrate_feature_eps(X, 6)
    else:
        eps = calibrate_eps(X, 10)
    gp = dict({"eps": eps, "k": 10 if "lambda_mode" not in extra else 6, "topk": 8, "p": 2.0, "sigma": None}, **extra)
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(4)
    taus = [1.0, 0.62, 0.0]
    for _ in range(3):
        q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.02 * rng.standard_normal(d) / np.sqrt(d))
        c0 = aspace.sweep_counters()
        got = aspace.search_taus(q, gl, taus)
        c1 = aspace.sweep_counters()
        assert c1["shared_passes"] == c0["shared_passes"]
        assert c1["taus_redone"] == c0["taus_redone"] + len(taus)
        for j, tau in enumerate(taus):
            same_as_single(got[j], aspace.search(q, gl, tau))


def test_crowded_neighbourhood_gives_the_single_searches_answers(oracle_lib):
    """cosine eps: 10 on x100-scaled rows (the reference's tests/test_3_beir.py:194): every item inside eps -- the k-NN
    buffer overflows, the pass is redone or takes the threshold repair; the answers stay the single searches'."""
    import arrowspace
    n, d = 5000, 64
    X = clustered(n, d, nclust=6, noise=0.4, seed=23, normalise=False) * 100.0
    gp = {"eps": 10.0, "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = arrowspace.ArrowSpaceBuilder.build(gp, X)
    ref = oracle_lib.OracleIndex(X, dict(gp, metric="cosine", kernel="rational"))
    rng = np.random.default_rng(9)
    for _ in range(4):
        q = np.ascontiguousarray(X[rng.integers(0, n)] * 1.02)
        check_sweep(aspace, gl, q, [1.0, 0.8, 0.62], ref)
        check_sweep(aspace, gl, q, [0.62, 0.8, 0.42, 0.0], ref)
    c = aspace.sweep_counters()
    assert c["calls"] == 8 and c["taus_redone"] > 0, c   # (at least the first pass: more than CAND_CAP rows inside eps)


def test_duplicates_tied_at_the_threshold(oracle_lib):
    rng = np.random.default_rng(0)
    base = rng.standard_normal((6, 16))
    X = np.repeat(base, 50, axis=0)       # 300 rows, 6 distinct points x 50 copies: massive exact ties
    import pyarrowspace_amd as asp
    gp = {"eps": 0.5, "k": 5, "topk": 6, "p": 2.0, "sigma": 0.3}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    ref = oracle_lib.OracleIndex(X, gp)
    for q in (base[2] + 0.01, base[5], base[0] * 1.001):
        q = np.ascontiguousarray(q)
        try:
            ref.search(q, 1.0)
        except oracle_lib.ZeroLambda:
            with pytest.raises(asp.PanicException):
                aspace.search_taus(q, gl, [1.0, 0.62, 0.0])
            continue
        check_sweep(aspace, gl, q, [1.0, 0.62, 0.3, 0.0], ref)


def test_zero_lambda_panics_exactly_when_search_does(oracle_lib):
    import pyarrowspace_amd as asp
    X = clustered(800, 32, nclust=8, seed=4)
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    far = np.ascontiguousarray(np.full(32, 50.0))   # no item within eps: lambda_q == 0
    near = np.ascontiguousarray(X[3] * 1.01)
    for q in (far, near):
        try:
            aspace.search(q, gl, 0.62)
            panics = False
        except asp.PanicException as e:
            panics, msg = True, str(e)
        if panics:
            with pytest.raises(asp.PanicException) as ei:
                aspace.search_taus(q, gl, [1.0, 0.62, 0.0])
            assert str(ei.value) == msg
            with pytest.raises(asp.PanicException):
                aspace.search_taus(q, gl, [2.0, 0.5])
        else:
            check_sweep(aspace, gl, q, [1.0, 0.62, 0.0])
    with pytest.raises(asp.PanicException):
        aspace.search(far, gl, 1.0)


def test_sweep_beside_concurrent_single_searches():
    import pyarrowspace_amd as asp
    n, d = 30000, 128
    X = clustered(n, d, nclust=64, seed=31)
    gp = {"eps": calibrate_eps(X, 10), "k": 10, "topk": 10, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(12)
    Q = [np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d)) for _ in range(6)]
    taus = [1.0, 0.8, 0.62, 0.0]
    serial_sweep = [aspace.search_taus(q, gl, taus) for q in Q]
    serial = [[aspace.search(q, gl, t) for t in taus] for q in Q]
    for a, b in zip(serial_sweep, serial):
        for x, y in zip(a, b):
            same_as_single(x, y)
    errors = []

    def sweeper():
        try:
            for _ in range(8):
                for q, want in zip(Q, serial_sweep):
                    assert aspace.search_taus(q, gl, taus) == want
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    def single(off):
        try:
            for r in range(8):
                for i in range(len(Q)):
                    qi = (i + off + r) % len(Q)
                    tj = (i + off) % len(taus)
                    assert aspace.search(Q[qi], gl, taus[tj]) == serial[qi][tj]
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=sweeper)] + [threading.Thread(target=single, args=(o,)) for o in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]


def test_headline_size_sweep_equals_single_searches():
    import pyarrowspace_amd as asp
    import bench
    n, d, k, topk = 1_000_000, 768, 25, 15
    X = gpu_clustered(n, d, 42)
    gp = {"eps": bench.calibrate_eps(X, k, "l2"), "k": k, "topk": topk, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    rng = np.random.default_rng(21)
    rows = rng.integers(0, n, 16)
    Xq = X[torch_rows(X, rows)].cpu().double().numpy()
    del X
    taus = [1.0, 0.8, 0.62, 0.42, 0.2, 0.0]
    c0 = aspace.sweep_counters()
    for i in range(16):
        q = np.ascontiguousarray(Xq[i] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        got = aspace.search_taus(q, gl, taus)
        for j, tau in enumerate(taus):
            same_as_single(got[j], aspace.search(q, gl, tau))
    c1 = aspace.sweep_counters()
    assert c1["shared_passes"] - c0["shared_passes"] == 16, (c0, c1)
    assert c1["taus_redone"] == c0["taus_redone"], (c0, c1)
