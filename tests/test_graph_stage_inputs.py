"""CPU: the hand-built inputs of tests/test_gpu_graph_stage.py are what that file takes them for.  For every case: the
oracle's outputs are finite, no weight underflows, no edge energy sits near its noise floor (where an ulp decides between a
value and 0), an ulp on every weight moves no output by more than 1e-11 (so the GPU test's 1e-9 keeps two orders of margin),
and the oracle's shard functions reproduce its whole graph's rows exactly.  The energy vectors of the median test hit the
ranks, ties, byte patterns and clamps they are named after."""
import numpy as np
import pytest

import test_gpu_graph_stage as gs
from oracle import oracle_np

COND_BOUND = 1e-11


def _case_id(case):
    return "-".join(str(c) for c in case)


def _energy_terms(ref):
    """Per CSR entry: edge_energy's value before the floor test, and the floor (oracle_np.edge_energy restated on arrays)."""
    prm, indptr, col = ref["prm"], ref["indptr"], ref["indices"]
    row = np.repeat(np.arange(len(ref["deg"])), np.diff(indptr))
    w, dist, g, ny = ref["w"], ref["dist"], ref["gy"], ref["ny"]
    alpha, beta = 1.0 / np.sqrt(ref["deg"][row]), 1.0 / np.sqrt(ref["deg"][col])
    nyi, nyj = ny[row], ny[col]
    if prm["metric"] == oracle_np.METRIC_L2:
        core = alpha * beta * (dist * dist) + (alpha - beta) * (alpha * nyi - beta * nyj)
    else:
        core = np.where((nyi > 0) & (nyj > 0), (alpha - beta) ** 2 + 2.0 * alpha * beta * (1.0 - g), alpha * alpha * nyi + beta * beta * nyj)
    floor = w * oracle_np.ENERGY_NOISE * (alpha * alpha * nyi + beta * beta * nyj + 2.0 * alpha * beta * np.abs(g))
    return w * core, floor


def _rel(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(a - b) / np.abs(b)
    r[a == b] = 0.0
    return float(np.max(r))


def _moved_weights(monkeypatch, seed):
    """oracle_np's edge weights, every one moved by one ulp (up or down at random)."""
    orig = oracle_np._edge_weight
    rng = np.random.default_rng(seed)

    def moved(d, sigma, p, kernel):
        w = np.asarray(orig(d, sigma, p, kernel), dtype=np.float64)
        return np.nextafter(w, np.where(rng.integers(0, 2, w.shape) == 1, np.inf, -np.inf))

    monkeypatch.setattr(oracle_np, "_edge_weight", moved)


def _cuts(case, n):
    if case[0] == "hubs":
        return gs.HUB_CUTS
    return sorted({0, n // 3, min(n, n // 3 + 1), n})


@pytest.mark.parametrize("case", gs.CASES, ids=_case_id)
def test_case_is_finite_well_conditioned_and_shards_reproduce_it(case, monkeypatch):
    X, gp, n64, lists = gs.graph_case(*case)
    prm = oracle_np.resolve_params(gp)
    n, k = X.shape[0], gp["k"]
    ref = gs.oracle_graph(case)
    for i, (js, key, _, _) in enumerate(lists):          # what the whole-graph routes assume and do not check
        assert len(js) <= k and i not in js and len(set(js.tolist())) == len(js)
        assert len(js) == 0 or (0 <= js.min() and js.max() < n)
        assert np.array_equal(np.lexsort((js, key)), np.arange(len(js)))
        assert (key <= oracle_np._eps_key(prm["eps"], prm["metric"])).all()
    for name in ("w", "lap", "deg", "E", "G", "lambdas"):
        assert np.isfinite(ref[name]).all(), name
    assert np.isfinite(ref["tau0"])
    if len(ref["w"]):
        assert ref["w"].min() >= np.finfo(np.float64).tiny
        v, floor = _energy_terms(ref)
        near = (v > 0.25 * floor) & (v < 4.0 * floor)
        assert not near.any(), (v[near], floor[near])
    # the shards of the oracle are its whole graph, exactly
    cuts = _cuts(case, n)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        r, s, dd, gg = gs.incoming_edges(lists, lo, hi)
        sh = oracle_np.shard_csr(prm, lo, hi - lo, lists[lo:hi], zip(r, s, dd, gg))
        E, G = oracle_np.shard_energy(sh, ref["deg"], n64)
        a, b = ref["indptr"][lo], ref["indptr"][hi]
        assert np.array_equal(sh["indptr"], ref["indptr"][lo : hi + 1] - a)
        assert np.array_equal(sh["indices"], ref["indices"][a:b])
        for name in ("dist", "gy", "w", "lap"):
            assert np.array_equal(sh[name], ref[name][a:b]), name
        assert np.array_equal(sh["deg"], ref["deg"][lo:hi])
        assert np.array_equal(E, ref["E"][lo:hi]) and np.array_equal(G, ref["G"][lo:hi])
    # an ulp on every weight
    _moved_weights(monkeypatch, 7)
    alt = oracle_np.graph_from_lists(X, prm, n64, lists)
    assert np.array_equal(alt["indices"], ref["indices"])
    worst = max(_rel(alt[name], ref[name]) for name in ("lap", "deg", "E", "G", "lambdas"))
    worst = max(worst, _rel(alt["tau0"], ref["tau0"]))
    assert worst < COND_BOUND, worst


def test_hub_case_has_its_hubs_and_its_empty_rows():
    for ps in gs.PARAM_SETS:
        X, gp, _, lists = gs.graph_case("hubs", *ps)
        ref = gs.oracle_graph(("hubs",) + ps)
        rowlen = np.diff(ref["indptr"])
        cnt = np.array([len(l[0]) for l in lists])
        assert X.shape == (4100, gs.D) and gp["k"] == 8
        assert rowlen.max() > 2000 and rowlen[0] > 2000 and cnt[0] == 0          # a hub through reverse entries alone
        assert rowlen[2050] > 2000 and rowlen[4099] > 2000
        assert int((rowlen == 0).sum()) > 30
        assert int(((cnt == 0) & (rowlen > 0)).sum()) > 100                      # rows that exist only through reverse entries
        mutual = sum(1 for t in range(0, 2050, 4) if 2 * t + 1 in lists[2 * t][0] and 2 * t in lists[2 * t + 1][0])
        assert mutual > 100
        one_sided = sum(1 for i, l in enumerate(lists) for j in l[0] if i not in lists[int(j)][0])
        assert one_sided > 1000
        assert cnt.max() == 8 and set(np.unique(cnt)) == set(range(9))


def test_special_cases_are_what_they_claim():
    for metric, kernel in (("l2", "gaussian"), ("cosine", "rational")):
        ref = gs.oracle_graph(("duplicates", metric, kernel, 2.0))
        X = ref["X"]
        assert np.array_equal(X[0], X[1]) and np.array_equal(X[2], X[3]) and np.array_equal(X[4], X[5])
        assert ref["deg"][0] == ref["deg"][1] and ref["E"][0] == 0.0 and ref["G"][0] == 0.0 and ref["lambdas"][1] == 0.0
        assert ref["deg"][2] != ref["deg"][3] and ref["E"][2] > 0.0 and ref["E"][3] > 0.0
        assert ref["deg"][4] != ref["deg"][5] and ref["E"][4] > 0.0 and ref["E"][5] > 0.0
        ref = gs.oracle_graph(("norms", metric, kernel, 2.0))
        norms = np.sqrt(ref["n"])
        assert norms[17] == 0.0 and ref["deg"][17] > 0.0 and ref["E"][17] == 0.0
        rest = np.delete(norms, 17)
        assert rest.min() >= 0.5 and rest.max() <= 2.0 and rest.max() / rest.min() > 2.0
        if metric == "l2":
            assert not np.allclose(ref["ny"], 1.0)
    ref = gs.oracle_graph(("empty", "l2", "gaussian", 2.0))
    assert len(ref["indices"]) == 0 and ref["tau0"] == oracle_np.TAU_MIN and not ref["lambdas"].any()
    ref = gs.oracle_graph(("wide", "l2", "gaussian", 2.0))
    assert ref["prm"]["k"] == 64 and max(len(j) for j in ref["knn"]) == 64 and min(len(j) for j in ref["knn"]) == 0


def test_median_shard_is_well_conditioned(monkeypatch):
    X, gp, n64, lists = gs.median_shard_inputs()
    prm = oracle_np.resolve_params(gp)
    ref = oracle_np.graph_from_lists(X, prm, n64, lists)
    assert (ref["E"] > 0).all() and (ref["G"] > 0).all() and (np.diff(ref["indptr"]) == 3).all()
    v, floor = _energy_terms(ref)
    assert (v > 4.0 * floor).all()
    _moved_weights(monkeypatch, 9)
    alt = oracle_np.graph_from_lists(X, prm, n64, lists)
    assert max(_rel(alt[name], ref[name]) for name in ("lap", "deg", "E", "G")) < COND_BOUND


def test_energy_vectors_hit_what_they_are_named_after():
    names = set()
    for n in gs.MEDIAN_SIZES:
        for name, E in gs.median_vectors(n):
            names.add(name)
            assert E.shape == (n,)
            pos = np.sort(E[E > 0])
            tau = oracle_np.median_tau(E)
            if name in ("zeros", "negatives", "nan", "mixed_nonpositive"):
                assert len(pos) == 0 and tau == 1e-12
            if name.endswith("_positive") and name[0].isdigit():
                c = int(name.split("_")[0])
                assert len(pos) == c and tau == pos[(c - 1) // 2]
                assert len(pos) < n or n <= 5
            if name.startswith("last_bytes"):
                b = pos.view(np.uint64)
                assert len(pos) in (299, 300) and (np.diff(b) == 1).all()
                assert len(set((b >> 16).tolist())) == 1 and len(set((b >> 8).tolist())) >= 2        # passes 7 and 8 decide
                assert tau == pos[(len(pos) - 1) // 2]
            if name == "tie_across_rank":
                assert tau == 0.25 and pos[(len(pos) - 1) // 2 - 1] == 0.25 and pos[(len(pos) - 1) // 2 + 1] == 0.25
            if name in ("tie_m_m", "tie_m1_m"):
                assert tau == 0.25 and pos[(len(pos) - 1) // 2 + 1] == 0.26       # the rank is the last a
            if name == "tie_m_m1":
                assert tau == 0.26 and pos[(len(pos) - 1) // 2 - 1] == 0.25       # the rank is the first b
            if name in ("clamp_low", "just_below_tau_min"):
                assert 0.0 < pos[(len(pos) - 1) // 2] < 1e-12 and tau == 1e-12
            if name == "clamp_high":
                assert pos[(len(pos) - 1) // 2] > 1.0 and tau == 1.0
            if name in ("wide_range", "clamp_low", "clamp_high"):
                assert pos[0] == 5e-324 and (pos < np.finfo(np.float64).tiny).sum() >= 2         # denormals take part
            if name == "positives_beyond_one_grid":
                assert n > 1024 * 256 and not (E[: 1024 * 256] > 0).any() and len(pos) == n - 1024 * 256 and len(pos) % 2 == 1
    assert {"zeros", "2_positive", "5_positive", "last_bytes_300", "tie_across_rank", "tie_m_m", "tie_m_m1", "wide_range", "clamp_low",
            "clamp_high", "positives_beyond_one_grid"} <= names
