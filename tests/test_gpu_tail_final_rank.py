"""GPU: the fused tail of a single search with the k-NN ranking in its FINAL kernel (staged_x1_final_kernel ranks the entries
inside eps that the blocks of staged_x1_kernel appended; as_set_tuning("x1_final_rank", 1), the default) against the fp64
oracle and, bit for bit, against the same searches with the ranking in the first kernel's last block ("x1_final_rank" 0): hits,
scores and lambda_q.  The order of the records, and with it every sum, does not depend on who ranks.

Data (make_data): 6 000 clustered unit rows of 64 columns (conftest.clustered) plus hand-placed groups, each a tight core
around a centre of its own (the rows inside eps of a query at that centre: P = the core's size, counted in fp64 by
tests/test_tail_final_rank_inputs.py) and a halo of 64 rows at cosine 0.7 to the centre -- outside eps, but enough rows near
the top of the cosine order that the scan's scorer bound settles above the background.  12 938 x 64 (the 6 000 rows, the groups'
6 298, ten halos) was the first shape run, and every case marked `fused` below was served there by the coarse scan
("int8-high") and the two-launch tail without a rerun; nothing smaller was tried -- the groups alone are half of it.

Cases: P = 0, k - 3, k, k + 1 (ranked as they are: P <= 64), 300 and 1 300 (the selection's histogram; more than one entry per
ranking thread), pairs of duplicate rows (keys tie, ids decide), 40 and 100 copies of one row with the query on it (every key equal:
kmax == kmin), k = 1 with topk = 1, k = 120, both metrics, tau 0.4 / 0.62 / 1, 4 500 rows inside eps (more than the candidate
buffer holds: the overflow chain answers), a sequence of searches on one workspace with a zero-lambda query in between, and
the two callers of the last-block form (a tau sweep, the coarse chain at tau = 0.2).  topk = 500 -- more hits than the
query's group and halo hold -- is not served by the fused tail on this index (the cosine window would have to take in the
background: the scan's scorer candidates overflow and the threshold chain answers); the case checks the answer only.
2 500 copies of one row with the query on it ("dups2500": they and the halo fit the candidate buffers, and every score falls
into one bin of the final kernels' histogram -- more entries than their pruned list, PRUNE_CAP = 2 048, holds, so the tail hands
the query on) in a single search and in a tau sweep: the cases check the answers, not the path.  (Where they were first run,
the search counter that moved was rerun_score_check -- 2 500 equal scores cannot be proven at the cut -- and neither
rerun_overflow nor rerun_knn_check; the sweep redid its three taus, shared_passes stayed 0.  The library's debug lines showed
the final kernel's overflow bit with 2 500 candidates written and nothing else that did not fit.)"""
import functools
import os

import numpy as np
import pytest

from conftest import assert_hits_match, calibrate_eps, clustered

pytestmark = pytest.mark.gpu

RTOL = 1e-9      # the project's bar (tests/test_gpu_parity.py)
D = 64
NBASE = 6000
HALO = 64
CAND_CAP = 4096  # the scan's candidate buffer (as_query.hpp)
COARSE_COEF_MAX = 4e-2   # the largest error coefficient the coarse scan accepts (query_begin)

# group name -> rows of its core; "pairs": 15 rows, each twice; "dups" / "dups100": one row 40 / 100 times (ranked as they are /
# through the selection, whose histogram then has one bin); "dups2500": one row 2 500 times (more than the pruned list of the final
# kernels holds; last, so that the rows of the groups before it are what they were without it)
GROUPS = {"none": 0, "lt_k": 7, "eq_k": 10, "k_plus_1": 11, "mid": 300, "dense": 1300, "pairs": 30, "dups": 40, "crowd": 4500, "dups100": 100,
          "dups2500": 2500}
PRUNE_CAP = 2048   # the pruned list of the final kernels (as_search.hip)
# index name -> (metric, k, topk)
# (the "crowd" and "dups2500" searches leave their workspace's path hints set -- the next 63 searches skip the prefilter --:
# indexes of their own)
INDEXES = {"l2": ("l2", 10, 8), "cosine": ("cosine", 10, 8), "l2_k1": ("l2", 1, 1), "l2_k120": ("l2", 120, 15), "l2_topk500": ("l2", 10, 500),
           "l2_crowd": ("l2", 10, 8), "cosine_crowd": ("cosine", 10, 8), "l2_dups2500": ("l2", 10, 8), "cosine_dups2500": ("cosine", 10, 8)}
# (index, group the query sits on, tau, served by the fused tail without a rerun)
CASES = [("l2", "none", 0.62, True), ("l2", "lt_k", 0.62, True), ("l2", "eq_k", 0.62, True), ("l2", "k_plus_1", 0.62, True),
         ("l2", "mid", 0.62, True), ("l2", "dense", 0.62, True), ("l2", "pairs", 0.62, True), ("l2", "dups", 0.62, True),
         ("l2", "dense", 1.0, True), ("l2", "mid", 0.4, True), ("l2", "dups100", 0.62, True),
         ("cosine", "none", 0.62, True), ("cosine", "lt_k", 0.62, True), ("cosine", "mid", 0.62, True), ("cosine", "dense", 0.62, True),
         ("cosine", "pairs", 0.62, True), ("cosine", "dups", 0.62, True), ("cosine", "dups100", 0.62, True),
         ("l2_k1", "dense", 0.62, True), ("l2_k1", "pairs", 0.62, True), ("l2_k1", "dups", 0.62, True),
         ("l2_k120", "k_plus_1", 0.62, True), ("l2_k120", "mid", 0.62, True), ("l2_k120", "dense", 0.62, True),
         ("l2_topk500", "lt_k", 0.62, False), ("l2_topk500", "dense", 0.62, False),
         ("l2_crowd", "crowd", 0.62, False), ("cosine_crowd", "crowd", 0.62, False),
         ("l2_dups2500", "dups2500", 0.62, False), ("cosine_dups2500", "dups2500", 0.62, False)]
ZERO_GROUP = "none"   # the one query per index with no row inside eps


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def make_data():
    """(X, {group: centre}, {group: (first core row, core rows)})"""
    rng = np.random.default_rng(2024)
    parts, centres, spans = [clustered(NBASE, D, nclust=16, seed=3)], {}, {}
    at = NBASE
    for name, size in GROUPS.items():
        c = _unit(rng.standard_normal(D))
        if name.startswith("dups"):
            core = np.repeat(c[None, :], size, axis=0)
        elif name == "pairs":
            half = _unit(c[None, :] + 0.02 * rng.standard_normal((size // 2, D)) / np.sqrt(D))
            core = np.concatenate([half, half])
        else:
            core = _unit(c[None, :] + 0.02 * rng.standard_normal((size, D)) / np.sqrt(D))
        o = rng.standard_normal((HALO, D))
        o = _unit(o - (o @ c)[:, None] * c[None, :])
        halo = 0.7 * c[None, :] + np.sqrt(1.0 - 0.49) * o
        parts += [core, halo]
        centres[name] = np.ascontiguousarray(c)
        spans[name] = (at, size)
        at += size + HALO
    X = np.ascontiguousarray(np.concatenate(parts))
    X.setflags(write=False)
    return X, centres, spans


@functools.lru_cache(maxsize=None)
def graph_params(index):
    metric, k, topk = INDEXES[index]
    base = make_data()[0][:NBASE]
    return {"eps": calibrate_eps(base, min(k, 40), metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric}


def query_of(group):
    return make_data()[1][group].copy()


_built = {}


def _index(index, oracle_lib):
    if index not in _built:
        import pyarrowspace_amd as asp
        X = make_data()[0]
        gp = graph_params(index)
        aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
        _built[index] = (aspace, gl, oracle_lib.OracleIndex(X, gp))
    return _built[index]


@pytest.fixture(autouse=True)
def _probe_coarse_and_restore_switch():
    import pyarrowspace_amd as asp
    os.environ["ARROWSPACE_SCAN_COARSE"] = "2"    # (every search probes the coarse scan, whatever the last one did)
    try:
        yield
    finally:
        os.environ.pop("ARROWSPACE_SCAN_COARSE", None)
        assert asp._L.as_set_tuning(b"x1_final_rank", -1) == 0   # (back to the workspaces' own switch)


def _search(aspace, gl, q, tau, final_rank):
    """hits, or None where the search panics (lambda_q = 0), and lambda_q, with the ranking where final_rank says"""
    import pyarrowspace_amd as asp
    assert asp._L.as_set_tuning(b"x1_final_rank", final_rank) == 0
    try:
        hits = aspace.search(q, gl, tau)
    except asp.PanicException:
        hits = None
    op = aspace.last_scan_operand
    return hits, aspace.query_lambda(q, gl), op


def _want(ref, oracle_lib, q, tau):
    try:
        want, lq = ref.search(q, tau)
    except oracle_lib.ZeroLambda:
        return None, 0.0
    return want, lq


@pytest.mark.parametrize("index,group,tau,fused", CASES)
def test_final_kernel_ranking_matches_oracle_and_last_block_form(oracle_lib, index, group, tau, fused):
    aspace, gl, ref = _index(index, oracle_lib)
    q = query_of(group)
    want, lq = _want(ref, oracle_lib, q, tau)
    c0 = aspace.search_counters()
    new, lq_new, op_new = _search(aspace, gl, q, tau, 1)
    c1 = aspace.search_counters()
    old, lq_old, op_old = _search(aspace, gl, q, tau, 0)
    print(f"{index} {group} tau={tau}: operand {op_new}/{op_old}, counters {c0} -> {c1}, lambda_q {lq_new!r} (oracle {lq!r}), "
          f"hits {None if new is None else len(new)}")
    assert new == old and lq_new == lq_old            # bit for bit
    if want is None:
        assert group == ZERO_GROUP and new is None and lq_new == 0.0
        assert c1["zero_lambda"] > c0["zero_lambda"]
    else:
        assert group != ZERO_GROUP
        assert_hits_match(new, want, ref.scores(q, tau, lq), rtol=RTOL)
        assert abs(lq_new - lq) <= RTOL * abs(lq)
        assert all(a[0] < b[0] for a, b in zip(new, new[1:]) if a[1] == b[1])   # ids ascending among equal scores
    if fused:
        assert op_new == op_old == "int8-high"
        assert c1["searches_with_rerun"] == c0["searches_with_rerun"], (c0, c1)


def test_state_is_cleared_between_searches_on_one_workspace(oracle_lib):
    """Three queries back to back, a zero-lambda query, the first one again: each answer is the one a freshly built index gives
    to that query as its first search -- what the final kernel clears for the next pass (the entries' counters, knn_total,
    knn_inexact) is cleared."""
    import pyarrowspace_amd as asp
    X = make_data()[0]
    gp = graph_params("l2")
    seq = ["dense", "lt_k", "pairs", ZERO_GROUP, "dense", "mid"]
    fresh = {}
    for g in set(seq):
        a2, g2 = asp.ArrowSpaceBuilder.build(gp, X)
        fresh[g] = _search(a2, g2, query_of(g), 0.62, 1)[:2]
        del a2, g2
    aspace, gl, ref = _index("l2", oracle_lib)
    c0 = aspace.search_counters()
    for g in seq:
        got = _search(aspace, gl, query_of(g), 0.62, 1)
        assert got[:2] == fresh[g], g
        assert got[2] == "int8-high"
    c1 = aspace.search_counters()
    assert c1["searches_with_rerun"] == c0["searches_with_rerun"] and c1["zero_lambda"] == c0["zero_lambda"] + 2


@pytest.mark.parametrize("index", ["l2", "cosine"])
def test_last_block_callers_are_unchanged(oracle_lib, index):
    """The tau sweep and the coarse chain (tau = 0.2) need lambda_q between the two block launches: their first launch still ranks
    in its last block, through the same ranking function -- same answers as the oracle's, whatever the switch says."""
    aspace, gl, ref = _index(index, oracle_lib)
    import pyarrowspace_amd as asp
    taus = [1.0, 0.8, 0.62]
    for g in ("mid", "pairs", "dense"):
        q = query_of(g)
        got = {}
        for sw in (1, 0):
            assert asp._L.as_set_tuning(b"x1_final_rank", sw) == 0
            got[sw] = (aspace.search_taus(q, gl, taus), aspace.search(q, gl, 0.2), aspace.last_scan_operand)
        assert got[0] == got[1]
        print(f"{index} {g}: chain operand {got[1][2]}, sweep {aspace.sweep_counters()}")
        for t, hits in zip(taus + [0.2], got[1][0] + [got[1][1]]):
            want, lq = ref.search(q, t)
            assert_hits_match(hits, want, ref.scores(q, t, lq), rtol=RTOL)


@pytest.mark.parametrize("index", ["l2_dups2500", "cosine_dups2500"])
def test_mass_tie_in_a_tau_sweep(oracle_lib, index):
    """The "dups2500" query under three taus at once, as the first call on an index of its own (no path hints yet: the shared
    pass runs): each list is search()'s for that tau (test_gpu_tau_sweep's rule: the same ids in the same order except where
    scores tie to 1e-12) and the oracle's."""
    import pyarrowspace_amd as asp
    from test_gpu_tau_sweep import same_as_single
    ref = _index(index, oracle_lib)[2]
    aspace, gl = asp.ArrowSpaceBuilder.build(graph_params(index), make_data()[0])
    q = query_of("dups2500")
    taus = [1.0, 0.62, 0.4]
    c0, s0 = aspace.search_counters(), aspace.sweep_counters()
    got = aspace.search_taus(q, gl, taus)
    c1, s1 = aspace.search_counters(), aspace.sweep_counters()
    print(f"{index} dups2500 sweep: counters {c0} -> {c1}, sweep {s0} -> {s1}")
    assert len(got) == len(taus)
    for tau, hits in zip(taus, got):
        same_as_single(hits, aspace.search(q, gl, tau))
        want, lq = ref.search(q, tau)
        assert_hits_match(hits, want, ref.scores(q, tau, lq), rtol=RTOL)
        assert all(a[0] < b[0] for a, b in zip(hits, hits[1:]) if a[1] == b[1])
