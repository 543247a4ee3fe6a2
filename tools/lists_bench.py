"""Per-query candidate lists at the headline size: `search_batch_lists` / `score_lists_batch` for B queries with C candidates each,
against what a caller had before -- the loop of `search_subset` / `score_items` single calls over the same lists, and
`score_items_batch` over the union of the lists.
python tools/lists_bench.py [N] [D] [OUT]  (defaults 1M x 768, profiles/r11_lists.txt).

Data, queries and parameters are those of tools/subset_batch_bench.py (clustered Gaussians by the torch RNG, seed 42; L2 /
Gaussian, k = 25, topk = 15, tau = 0.62; bench.make_queries, seed 43).  Cases: (B, C) in {(1024, 100), (1024, 1000), (128, 10000)}
with every list drawn uniformly without replacement (seed 45), and one ragged case of 1024 lists with lengths log-uniform in
[10, 10000].  Every case's lists are checked first against `search_subset` (the first 8 and last 8 queries) with
`same_as_single`.  Per case, medians of REPS calls: the two list forms per query; the loops of single calls on 64 of the queries;
`score_items_batch` for those 64 queries over the union of ALL the case's lists (one tile of the batched kernel: its per-query
cost does not fall with more queries); `search_batch` alone (the lambda_q step); the ragged score kernel's device time by HIP
events and its gather rate sum(m_i) x dp x 4 bytes / time beside `subset_score_kernel`'s rate over all N rows measured in the
same process; and the host share (id checks, deduplication, work tables: `lists_counters()['host_ns']`)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from subset_bench import same_as_single  # noqa: E402
from tau_sweep_bench import gpu_clustered  # noqa: E402

REPS = 5
NSINGLE = 64


def draw_list(rng, n, c):
    """c distinct ids, uniform, in random order (without a permutation of all n per list)"""
    c = min(c, n)
    u = np.unique(rng.integers(0, n, c + c // 8 + 16))
    while len(u) < c:
        u = np.unique(np.concatenate([u, rng.integers(0, n, c)]))
    return rng.permutation(u)[:c].astype(np.int64)


def med_us(f, reps=REPS):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts))


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    out = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "r11_lists.txt")
    X = gpu_clustered(n, d, 42)
    gp = {"eps": bench.calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = np.ascontiguousarray(np.stack([np.ascontiguousarray(q) for q in bench.make_queries(X, 1024, 43)]))
    del X
    torch.cuda.synchronize()
    dp = (d + 31) // 32 * 32
    tau = 0.62
    rng = np.random.default_rng(45)
    # the single kernel's gather rate over all N rows (the same row bytes per entry)
    full = aspace.subset(np.arange(n))
    full.set_timing(True)
    ks = []
    for i in range(8):
        aspace.search_subset(np.ascontiguousarray(Q[i]), gl, tau, full)
        ks.append(full.kernel_us)
    del full
    single_rate = n * dp * 4 / (float(np.median(ks[2:])) * 1e-6) / 1e12
    lines = [f"search_batch_lists / score_lists_batch: N={n} D={d} k=25 topk=15 l2/gaussian eps={gp['eps']:.5f} tau={tau}; medians of {REPS} calls; "
             f"kernel = lists_score_kernel by HIP events, summed over the chunks of a call; rate = sum(m_i) x {dp} x 4 bytes / kernel time; "
             f"subset_score_kernel over all {n} rows in this process: {float(np.median(ks[2:])):.1f} us = {single_rate:.2f} TB/s"]
    print(lines[0], flush=True)
    cases = [(f"B=1024 C=100", 1024, lambda: 100), ("B=1024 C=1000", 1024, lambda: 1000), ("B=128 C=10000", 128, lambda: 10000),
             ("B=1024 ragged 10..10000", 1024, lambda: int(round(10.0 ** rng.uniform(1.0, 4.0))))]
    for name, b, length in cases:
        Qb = np.ascontiguousarray(Q[:b])
        lists = [draw_list(rng, n, length()) for _ in range(b)]
        total = int(sum(len(l) for l in lists))
        arg = np.stack(lists) if len({len(l) for l in lists}) == 1 else lists
        got = aspace.search_batch_lists(Qb, gl, tau, arg)   # warm-up (the buffers are made here), and the lists
        rows = aspace.score_lists_batch(Qb, gl, tau, arg)
        for i in list(range(8)) + list(range(b - 8, b)):
            qi = np.ascontiguousarray(Qb[i])
            same_as_single(got[i], aspace.search_subset(qi, gl, tau, lists[i]))
            np.testing.assert_allclose(rows[i], aspace.score_items(qi, gl, tau, lists[i]), rtol=1e-12, atol=0.0)
        assert asp._L.as_set_tuning(b"lists_timing", 1) == 0
        try:
            c0 = aspace.lists_counters()
            t_search = med_us(lambda: aspace.search_batch_lists(Qb, gl, tau, arg))
            c1 = aspace.lists_counters()
            ku = []
            t_score = med_us(lambda: (aspace.score_lists_batch(Qb, gl, tau, arg), ku.append(asp._L.as_lists_kernel_us(aspace._h))))
            c2 = aspace.lists_counters()
        finally:
            assert asp._L.as_set_tuning(b"lists_timing", 0) == 0
        t_sb = med_us(lambda: aspace.search_batch(Qb, gl, tau))
        host_search = (c1["host_ns"] - c0["host_ns"]) / REPS / 1e3
        host_score = (c2["host_ns"] - c1["host_ns"]) / REPS / 1e3
        launches = (c2["score_launches"] - c1["score_launches"]) // REPS
        kus = float(np.median(ku))
        rate = total * dp * 4 / (kus * 1e-6) / 1e12
        sel = range(0, b, max(b // NSINGLE, 1))
        sel = list(sel)[:NSINGLE]
        t_loop_search = med_us(lambda: [aspace.search_subset(np.ascontiguousarray(Qb[i]), gl, tau, lists[i]) for i in sel], 3) / len(sel)
        t_loop_score = med_us(lambda: [aspace.score_items(np.ascontiguousarray(Qb[i]), gl, tau, lists[i]) for i in sel], 3) / len(sel)
        union = np.unique(np.concatenate(lists))
        Qs = np.ascontiguousarray(Qb[sel])
        t_union = med_us(lambda: aspace.score_items_batch(Qs, gl, tau, union), 3) / len(sel)
        lines.append(f"{name}: sum(m_i)={total} | search_batch_lists {t_search:.0f} us = {t_search / b:.1f} us/query | score_lists_batch "
                     f"{t_score:.0f} us = {t_score / b:.1f} us/query | search_batch alone {t_sb:.0f} us = {t_sb / b:.1f} us/query | loop of single "
                     f"calls ({len(sel)} queries): search_subset {t_loop_search:.1f} us/query, score_items {t_loop_score:.1f} us/query | "
                     f"score_items_batch over the union ({len(union)} ids, {len(sel)} queries) {t_union:.1f} us/query | score kernel {kus:.1f} us in "
                     f"{launches} launch(es) = {kus / b:.2f} us/query, {total * dp * 4 / 1e6:.1f} MB gathered = {rate:.2f} TB/s = "
                     f"{rate / single_rate:.2f} of the single kernel's rate | host share: search form {host_search:.0f} us = "
                     f"{host_search / t_search:.3f} of the call, score form {host_score:.0f} us = {host_score / t_score:.3f}")
        print(lines[-1], flush=True)
    lines.append(f"lists_counters {aspace.lists_counters()}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])


if __name__ == "__main__":
    main()
