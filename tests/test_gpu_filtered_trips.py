"""GPU: the later trips of the filtered family's stride loops.  Every grid of these kernels is clipped and finished by a loop
(subset_score_kernel, the radix select's passes, lists_score_kernel, fused_accumulate_kernel, group_pick_kernel,
range_compact_kernel), and at the shapes the suite can afford every block takes one trip.  as_set_tuning("filtered_grid_cap", v)
clips gridDim.x of those kernels to v blocks: with 1, 2 and 3 blocks every form's answer must be bit-equal to its answer with
the cap off, which is held against its numpy route here.  One case needs no hook: 1100 range queries in one chunk leave
range_compact_kernel one block per row, which takes three trips over 5000 scores.
Indexes: tests/test_gpu_grouped.py's 1500x51 and 3000x96cos, tests/test_gpu_subset.py's 5000x32 (test_topk_edges), and the
poisoned 3000x51 of tests/test_gpu_filtered_nonfinite.py."""
import numpy as np
import pytest

import fused_ref
import grouped_ref
import test_gpu_filtered_nonfinite as nf
import test_gpu_grouped as tg
from conftest import calibrate_eps, clustered

pytestmark = pytest.mark.gpu

TAUS = (1.0, 0.62, 0.0)
_wide = {}


def wide_index():
    """test_topk_edges' 5000x32: (asp, aspace, gl, X)."""
    if not _wide:
        import pyarrowspace_amd as asp
        X = clustered(5000, 32, nclust=16, seed=15)
        gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 1024, "p": 2.0, "sigma": None}
        _wide["ix"] = (asp, *asp.ArrowSpaceBuilder.build(gp, X), X)
    return _wide["ix"]


def canon(x):
    """A result as nested tuples in which floats are their bits, every NaN alike."""
    if isinstance(x, np.ndarray) and x.dtype == np.float64:
        nan = np.isnan(x)
        return (x.shape, nan.tobytes(), np.where(nan, 0.0, x).view(np.uint64).tobytes())
    if isinstance(x, np.ndarray):
        return (x.shape, x.tobytes())
    if isinstance(x, (float, np.floating)):
        return "nan" if x != x else int(np.float64(x).view(np.uint64))
    if isinstance(x, (list, tuple)):
        return tuple(canon(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, canon(v)) for k, v in x.items())
    return x


def capped(asp, cap, call):
    try:
        assert asp._L.as_set_tuning(b"filtered_grid_cap", cap) == 0
        return call()
    finally:
        assert asp._L.as_set_tuning(b"filtered_grid_cap", 0) == 0


def range_want(ids, s, thr):
    wi, ws = nf.range_want(ids, s, thr)
    return list(zip(wi.tolist(), ws.tolist()))


def every_form(aspace, gl, V, ids, labels, topk):
    """name -> answer of every filtered form over the ids (sorted, an odd number of them), each held against its numpy route."""
    m = len(ids)
    assert m % 2 == 1 and m > 1024
    sub = aspace.subset(ids)
    k = min(topk, m)
    q, Q3, Q65 = V[0], V[:3], V[:65]
    rng = np.random.default_rng(m)
    lists = [np.sort(rng.choice(ids, int(rng.integers(1, 1400)), replace=False))[::-1].copy() for _ in range(65)]
    out = {}
    # scores and selections: single, sweep, batched, lists
    out["score_items"] = s = aspace.score_items(q, gl, 0.62, ids)
    out["score_items_taus"] = st = aspace.score_items_taus(q, gl, TAUS, ids)
    nf.same_scores(st[1], s)
    out["search_subset"] = aspace.search_subset(q, gl, 0.62, sub)
    nf.same_hits(out["search_subset"], ids, s, k)
    out["search_subset_taus"] = aspace.search_subset_taus(q, gl, TAUS, sub)
    for u in range(len(TAUS)):
        nf.same_hits(out["search_subset_taus"][u], ids, st[u], k)
    out["score_items_batch"] = S = aspace.score_items_batch(Q65, gl, 0.62, ids)
    out["search_batch_subset"] = aspace.search_batch_subset(Q65, gl, 0.62, sub)
    for i in range(65):
        nf.same_hits(out["search_batch_subset"][i], ids, S[i], k)
    out["search_batch_subset_taus"] = aspace.search_batch_subset_taus(Q3, gl, TAUS, sub)
    ST = aspace.score_items_batch_taus(Q3, gl, TAUS, ids)
    for i in range(3):
        for u in range(len(TAUS)):
            nf.same_hits(out["search_batch_subset_taus"][i][u], ids, ST[i, u], k)
    out["score_lists_batch"] = SL = aspace.score_lists_batch(Q65, gl, 0.62, lists)
    out["search_batch_lists"] = aspace.search_batch_lists(Q65, gl, 0.62, lists)
    for i in range(65):
        nf.same_hits(out["search_batch_lists"][i], lists[i], SL[i], min(topk, len(lists[i])))
    out["score_lists_batch_taus"] = SLT = aspace.score_lists_batch_taus(Q3, gl, TAUS, lists[:3])
    out["search_batch_lists_taus"] = aspace.search_batch_lists_taus(Q3, gl, TAUS, lists[:3])
    for i in range(3):
        nf.same_scores(SLT[i][1], SL[i])
        for u in range(len(TAUS)):
            nf.same_hits(out["search_batch_lists_taus"][i][u], lists[i], SLT[i][u], min(topk, len(lists[i])))
    # range: single, batched over 65 rows, the counts
    thr = float(np.nanquantile(s, 0.7))
    out["search_range"] = aspace.search_range(q, gl, 0.62, thr, subset=sub)
    assert canon(out["search_range"]) == canon(range_want(ids, s, thr))
    out["count_range"] = aspace.count_range(q, gl, 0.62, thr, subset=sub)
    assert out["count_range"] == len(out["search_range"])
    thrs = [float(np.nanquantile(S[i], 0.5 + 0.007 * i)) if i % 9 else -np.inf for i in range(65)]
    out["search_range_batch"] = aspace.search_range_batch(Q65, gl, 0.62, thrs, subset=sub)
    for i in range(65):
        assert canon(out["search_range_batch"][i]) == canon(range_want(ids, S[i], thrs[i]))
    out["count_range_batch"] = aspace.count_range_batch(Q65, gl, 0.62, thrs, subset=sub)
    assert out["count_range_batch"].tolist() == [len(g) for g in out["search_range_batch"]]
    # fused
    for mode in ("sum", "max"):
        with np.errstate(all="ignore"):
            F = fused_ref.fuse(S[:3], [0.5, -0.25, 2.0], mode)
        out["score_fused " + mode] = aspace.score_fused(Q3, gl, 0.62, ids, weights=[0.5, -0.25, 2.0], mode=mode)
        nf.same_scores(out["score_fused " + mode], F)
        out["search_fused " + mode] = aspace.search_fused(Q3, gl, 0.62, weights=[0.5, -0.25, 2.0], mode=mode, subset=sub)
        nf.same_hits(out["search_fused " + mode], ids, F, k)
    # grouped: later rounds (per_group = 3; at most 1024 slots: the combining form) and more than 1024 groups (the plain form)
    single = np.arange(len(labels))
    assert len(np.unique(single[ids])) > 1024 >= len(np.unique(labels[ids]))
    for lname, lab in (("few", labels), ("singletons", single)):
        grp = aspace.groups(lab)
        for ng, pg in ((5, 3), (1024, 1)):
            got = aspace.search_grouped(q, gl, 0.62, grp, ng, pg, subset=sub)
            nf.same_groups(got, grouped_ref.grouped(ids, lab[ids], s, ng, pg))
            out[f"search_grouped {lname} {ng} {pg}"] = got
        res = aspace.search_batch_grouped(Q65, gl, 0.62, grp, 4, 3, subset=sub)
        for i in range(65):
            nf.same_groups(res[i], grouped_ref.grouped(ids, lab[ids], S[i], 4, 3))
        out[f"search_batch_grouped {lname}"] = res
    return out


def under_every_cap(asp, run):
    base = canon(run())
    for cap in (1, 2, 3):
        got = capped(asp, cap, run)
        for (name, a), (_, b) in zip(base, canon(got)):
            assert a == b, (cap, name)


@pytest.mark.parametrize("name", ["1500x51", "3000x96cos"])
def test_every_form_under_a_capped_grid(name):
    asp, X, gp, aspace, gl, V = tg.index(name)
    n = X.shape[0]
    ids = np.arange(1, n) if n % 2 == 0 else np.arange(n)
    under_every_cap(asp, lambda: every_form(aspace, gl, V, ids, np.arange(n) // 7, gp["topk"]))


def test_the_poisoned_fixture_under_a_capped_grid():
    asp, fx, gp, aspace, gl, V, ref = nf.index("3000x51")
    n = fx["X"].shape[0]
    ids = np.arange(1, n)
    labels = nf.grouped_labels(fx)["crafted"]
    under_every_cap(asp, lambda: every_form(aspace, gl, V, ids, labels, gp["topk"]))


def served_queries(aspace, gl, X, count):
    out = []
    for r in np.random.default_rng(3).permutation(X.shape[0]):
        q = np.ascontiguousarray(X[r] * 1.01)
        if aspace.query_lambda(q, gl) != 0.0:
            out.append(q)
            if len(out) == count:
                break
    assert len(out) == count
    return np.stack(out)


def test_range_rows_of_odd_length_under_a_capped_grid():
    """m = 2 x 2048 + 1: an odd row length flips the 16-byte alignment (`head`) from row to row, and one block takes three trips."""
    asp, aspace, gl, X = wide_index()
    ids = np.arange(300, 300 + 4097)
    sub = aspace.subset(ids)
    Q = served_queries(aspace, gl, X, 6)
    S = aspace.score_items_batch(Q, gl, 0.62, ids)
    thrs = [float(np.quantile(S[i], 0.3 + 0.1 * i)) for i in range(6)]

    def run():
        got = aspace.search_range_batch(Q, gl, 0.62, thrs, subset=sub)
        for i in range(6):
            assert canon(got[i]) == canon(range_want(ids, S[i], thrs[i]))
        cnt = aspace.count_range_batch(Q, gl, 0.62, thrs, subset=sub)
        assert cnt.tolist() == [len(g) for g in got]
        one = aspace.search_range(Q[1], gl, 0.62, thrs[1], subset=sub)
        assert canon(one) == canon(range_want(ids, aspace.score_items(Q[1], gl, 0.62, ids), thrs[1]))
        return {"batch": got, "counts": cnt, "single": one}

    under_every_cap(asp, run)


def test_eleven_hundred_range_queries_leave_one_block_per_row():
    """No hook: RC_BLOCKS / 1100 = 1, so each row's one block takes three trips of 2048 scores over the 5000 items."""
    asp, aspace, gl, X = wide_index()
    n, B = X.shape[0], 1100
    assert n >= 4100
    ids = np.arange(n)
    Q = served_queries(aspace, gl, X, B)
    S = aspace.score_items_batch(Q, gl, 0.62, ids)
    thrs = [-np.inf if i % 100 == 0 else float(np.quantile(S[i], 0.99 - 0.0002 * (i % 50))) for i in range(B)]
    c0 = aspace.range_counters()
    got = aspace.search_range_batch(Q, gl, 0.62, thrs)
    c1 = aspace.range_counters()
    assert c1["compactions"] - c0["compactions"] - (c1["relaunches"] - c0["relaunches"]) == 1   # one chunk: 1100 rows in one launch
    for i in range(B):
        assert canon(got[i]) == canon(range_want(ids, S[i], thrs[i]))
    assert aspace.count_range_batch(Q, gl, 0.62, thrs).tolist() == [len(g) for g in got]
