"""CPU: the hand-built records of tests/test_gpu_staged_records.py are what that file takes them for, on the oracle alone
(oracle_np.staged_lambda / staged_merge): a wrong tie-break moves lambda_q by at least 1e-6 relative -- 1 000 x the GPU bar,
so a wrong pick cannot hide under it; every non-degenerate case has lambda_q >= 1e-3 and every degenerate one exactly 0; the
sums are well conditioned (any summation order agrees to 1e-12, so the 1e-9 bar absorbs no ill-conditioned sum); no case
holds an id twice; and the two oracle functions return what the inline merges of tests/test_dist_gloo.py's engine returned
before they were replaced by them (tests/golden/staged_records_gloo.json, recorded from that code on that file's records)."""
import json
import os

import numpy as np
import pytest

import test_gpu_staged_records as sr
from oracle import oracle_np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def tau0_of(oracle_lib):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = float(oracle_lib.OracleIndex(*sr.config_data(name)).tau0)
        return cache[name]
    return get


def _valid(recs):
    return recs[oracle_np.rec_ids(recs) >= 0]


def _no_id_twice(recs):
    ids = oracle_np.rec_ids(recs)
    ids = ids[ids >= 0]
    assert len(np.unique(ids)) == len(ids) and (ids <= 10 ** 9).all()


@pytest.mark.parametrize("name", sr.LAMBDA_CONFIGS)
def test_lambda_cases_are_what_their_names_say(name, tau0_of):
    n, d, k, topk, metric, kernel, p, sigma, R = sr.CONFIGS[name]
    prm, q, tau0 = sr.prm_of(name), sr.case_query(name), tau0_of(name)
    nq = float(q @ q)
    assert 1e-12 < tau0 < 1.0
    cases = {c["name"]: c for c in sr.lambda_cases(name)}
    assert {"exactly_k", "many_more_than_k", "tie_pair_at_the_cut", "tie_run_of_3_across_the_cut", "item_identical_to_the_query", "m_0",
            "all_slots_empty", "edge_energies_zero", f"every_slot_valid_R{R}"} <= set(cases)
    assert ("fewer_than_k" in cases) == (k > 1) and ("weights_underflow" in cases) == (metric == "l2" and kernel == "gaussian")
    rng = np.random.default_rng(1)
    for c in cases.values():
        recs = c["recs"][: c["m"]]
        assert c["m"] <= sr.REC_CAP and (c["m"] == 0 or len(c["recs"]) % k == 0)
        _no_id_twice(recs)
        lam, kept = oracle_np.staged_lambda(prm, tau0, nq, recs, k)
        v = _valid(recs)
        assert len(kept) == min(k, len(v))
        if c["zero"]:
            assert lam == 0.0
            continue
        assert lam >= 1e-3
        assert np.isfinite(v).all() and (v[:, 4] > 0).all()
        if 4 <= len(v) < len(recs):     # empties anywhere, not only trailing: some valid record lies behind an empty slot
            ids = oracle_np.rec_ids(recs)
            assert np.nonzero(ids >= 0)[0].max() > np.nonzero(ids < 0)[0].min()
            assert set(np.unique(recs[ids < 0, 1][~np.isnan(recs[ids < 0, 1])]).tolist()) <= {0.0, -1.0, np.inf} and np.isnan(recs[ids < 0, 2]).all()
        # conditioning: the kept records summed in (key, id) order and in a random order
        o = sr.ranked(recs)[:k]
        for order in (o, o[rng.permutation(len(o))]):
            again = oracle_np.neighbour_lambda(prm, tau0, nq, recs[order, 2], recs[order, 3], recs[order, 4], recs[order, 5])
            assert abs(again - lam) <= 1e-12 * lam
        if c["tie"]:
            r = sr.ranked(recs)
            a, b = recs[r[k - 1]], recs[r[k]]
            assert a[1] == b[1] and oracle_np.rec_ids(recs)[r[k - 1]] < oracle_np.rec_ids(recs)[r[k]]       # the cut lies inside a run of equal keys
            assert a[4] != b[4]
            if metric == "l2":
                assert a[3] != b[3] or a[5] != b[5]
            assert r[k - 1] // k != r[k] // k or len(recs) // k == 1 or c["name"] != "tie_pair_at_the_cut"     # across rank blocks
            other = oracle_np.staged_lambda(prm, tau0, nq, sr.wrong_pick(recs, k), k)[0]
            assert abs(other - lam) >= 1e-6 * lam, (c["name"], lam, other)
        if c["name"] == "tie_run_of_3_across_the_cut":
            r = sr.ranked(recs)
            assert int((recs[r, 1] == recs[r[k - 1], 1]).sum()) >= 3
        if c["name"] == "item_identical_to_the_query":
            assert v[:, 2].min() == 0.0 and oracle_np.rec_ids(recs)[sr.ranked(recs)[0]] in kept
    full = cases[f"every_slot_valid_R{R}"]
    assert full["m"] == R * k and (oracle_np.rec_ids(full["recs"]) >= 0).all()
    if name == "k64":
        assert cases["capacity_1024"]["m"] == sr.REC_CAP and (oracle_np.rec_ids(cases["capacity_1024"]["recs"]) >= 0).all()
    if "weights_underflow" in cases:
        w = _valid(cases["weights_underflow"]["recs"])
        assert (oracle_np._edge_weight(w[:, 2], prm["sigma"], prm["p"], prm["kernel"]) == 0.0).all()
    z = _valid(cases["edge_energies_zero"]["recs"])
    a = oracle_np._edge_weight(z[:, 2], prm["sigma"], prm["p"], prm["kernel"])
    assert (a == 1.0).all() and all(oracle_np.edge_energy(1.0, prm["metric"], z[t, 2], z[t, 3], float(len(z)), z[t, 4] + 1.0,
                                                          nq if metric == "l2" else 1.0, z[t, 5]) == 0.0 for t in range(len(z)))


def test_configs_cover_what_the_issue_lists():
    C = sr.CONFIGS
    assert {(C[c][8], C[c][2]) for c in sr.LAMBDA_CONFIGS} >= {(1, 1), (2, 5), (3, 63), (2, 64), (2, 65), (8, 120)}
    assert {(C[c][4], C[c][5]) for c in sr.LAMBDA_CONFIGS} >= {("l2", "gaussian"), ("cosine", "rational")}
    assert any(C[c][6] != 2.0 and C[c][7] is not None for c in C)
    assert all(64 <= C[c][0] <= 300 and C[c][1] == 24 for c in sr.LAMBDA_CONFIGS) and C["cap"][:4] == (1100, 16, 6, 1024)
    assert {t for _, t in sr.HIT_CONFIGS} == {1, 15, 64, 1024} and all(C[c][3] == t for c, t in sr.HIT_CONFIGS)
    assert sr.HIT_CAP == 8 * (1024 + 1) + 8 and sr.REC_CAP == 1024


@pytest.mark.parametrize("name,nranks", [("k5", 1), ("k5", 3), ("k5", 8), ("k65", 3), ("k120", 8), ("k120c", 3)])
def test_batched_lambda_cases(name, nranks, tau0_of):
    k = sr.CONFIGS[name][2]
    prm, tau0 = sr.prm_of(name), tau0_of(name)
    Q, recs, flat, counts = sr.batch_lambda_case(name, nranks)
    assert recs.shape == (nranks, sr.SLOTS, k, 6) and len(Q) == 29 and nranks * k <= sr.REC_CAP
    assert {0, k} <= set(counts) and (len(set(counts)) == len(counts) or nranks * k + 1 < len(counts))
    ties = 0
    for b in range(sr.SLOTS):
        assert np.array_equal(recs[:, b].reshape(-1, 6), flat[b], equal_nan=True)           # flattened in rank order
        ids = oracle_np.rec_ids(flat[b])
        if b >= len(Q):
            assert (ids < 0).all()
            continue
        _no_id_twice(flat[b])
        assert int((ids >= 0).sum()) == counts[b]
        lam = oracle_np.staged_lambda(prm, tau0, float(Q[b] @ Q[b]), flat[b], k)[0]
        assert lam >= 1e-3 or (lam == 0.0 and counts[b] == 0)
        r = sr.ranked(flat[b])
        if len(r) > k and flat[b][r[k - 1], 1] == flat[b][r[k], 1]:
            ties += 1
            other = oracle_np.staged_lambda(prm, tau0, float(Q[b] @ Q[b]), sr.wrong_pick(flat[b], k), k)[0]
            assert abs(other - lam) >= 1e-6 * lam
    assert ties >= 3 or nranks * k <= k + 1


@pytest.mark.parametrize("topk,R", [(1, 1), (1, 8), (15, 2), (64, 8), (1024, 1), (1024, 8)])
def test_hit_cases_are_what_their_names_say(topk, R):
    rng = sr._rng("inputs", topk, R)
    m = R * (topk + 1)
    for kind in sr.HIT_KINDS:
        hits = sr.hit_case(kind, topk, m, R, rng, flags=(0,) * (R - 1))
        _no_id_twice(hits)
        ids, sc = oracle_np.rec_ids(hits), hits[:, 1]
        assert set(np.unique(ids[ids < 0]).tolist()) <= {-1, -2} and int((ids == -2).sum()) == R - 1
        assert (ids[: topk + 1] != -2).all() or R == 1
        assert (np.isnan(sc[ids == -1]) | np.isposinf(sc[ids == -1])).all()                 # empties that would win every ranking
        want, fl = oracle_np.staged_merge(hits, topk)
        nv = int((ids >= 0).sum())
        assert fl == 0 and len(want) == min(topk, nv)
        assert [w for w in want] == sorted(want, key=lambda w: (-w[1], w[0]))
        order = sorted(((-(s + 0.0), int(i)) for i, s in zip(ids[ids >= 0], sc[ids >= 0])))
        assert [i for _, i in order[:topk]] == [i for i, _ in want]
        if kind in ("tie_at_the_cut", "tie_run_across_the_cut"):
            assert nv > topk and order[topk - 1][0] == order[topk][0]
            blocks = {int(np.nonzero(ids == i)[0][0]) // (topk + 1) for s, i in order if s == order[topk][0]}
            assert len(blocks) > 1 or R == 1
        if kind == "tie_run_across_the_cut" and nv >= topk + 2:
            assert sum(1 for s, _ in order if s == order[topk][0]) >= 3
        if kind == "signed_zeros" and nv >= 3:
            z = sc[(ids >= 0) & (sc == 0.0)]
            assert np.signbit(z).any() and not np.signbit(z).all()
        if kind == "minus_inf_valid":
            assert np.isneginf(sc[ids >= 0]).any() and nv <= topk
        if kind == "fewer_than_topk":
            assert nv == topk // 2
    for flags in [(1,), (32,), (1, 2, 4, 8), (4, 4), ()]:
        if len(flags) > m - (topk + 1 if R > 1 else 0):
            continue
        hits = sr.hit_case("plain", topk, m, R, rng, flags=flags)
        assert oracle_np.staged_merge(hits, topk)[1] == int(np.bitwise_or.reduce(np.array(flags + (0,))))
    assert sr.flags_expected(1 | 8) == (1, 2) and sr.flags_expected(2 | 4) == (2, 1) and sr.flags_expected(16 | 32) == (0, 0)


def test_oracle_merges_return_what_the_gloo_engine_returned_inline():
    """tests/test_dist_gloo.py's engine on its own records (two row ranges of its 300 x 24 index), against the values its
    inline merges produced before they became oracle_np.staged_lambda / staged_merge."""
    import torch

    import test_dist_gloo as tg
    from conftest import calibrate_eps, clustered
    from pyarrowspace_amd.dist import ShardedIndex
    z = json.load(open(os.path.join(G, "staged_records_gloo.json")))
    X = clustered(z["n"], z["d"], nclust=z["nclust"], seed=z["seed"])
    gp = {"eps": calibrate_eps(X, z["k"]), "k": z["k"], "topk": z["topk"], "p": 2.0, "sigma": None}
    e = ShardedIndex.build(gp, torch.from_numpy(X), engine=tg.OracleEngine(gp)).engine
    rng = np.random.default_rng(z["qseed"])
    cuts = z["cuts"]
    for case in z["cases"]:
        q = X[rng.integers(0, z["n"])] + 0.02 * rng.standard_normal(z["d"]) / np.sqrt(z["d"])
        recs = []
        for r in range(len(cuts) - 1):
            e.query_scan(q, cuts[r], cuts[r + 1])
            recs.append(e.knn_local.numpy().copy())
        recs = np.concatenate(recs)
        lam, kept = oracle_np.staged_lambda(e.prm, e.index["tau0"], float(q @ q), recs, z["k"])
        assert lam.hex() == case["lambda_q"] and 1 <= len(kept) <= z["k"]
        e.lq = lam
        for tau in z["taus"]:
            hits = []
            for r in range(len(cuts) - 1):
                e.query_scan(q, cuts[r], cuts[r + 1])
                e.query_score(tau)
                hits.append(e.hits_local.numpy().copy())
            got, fl = oracle_np.staged_merge(np.concatenate(hits), z["topk"])
            assert fl == 0 and [[i, s.hex()] for i, s in got] == case["hits"][str(tau)]
