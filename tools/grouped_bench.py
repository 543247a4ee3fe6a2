"""Grouped search at the headline size: `search_grouped` / `search_batch_grouped` against the only route there was before them --
`score_items` (batched cell: `score_items_batch`) over the same ids to host memory, then the numpy group-by of
tests/grouped_ref.py -- per query, alternating in one process; `search_subset` over the same ids in the same process (the same
gather and the same selection: what grouping adds); the pick kernels' own duration by HIP events
(as_set_tuning("grouped_timing")) and the 64-bit max-atomics they issued (as_grouped_counters [3]).
python tools/grouped_bench.py [N] [D] [QUERIES] [ROUNDS] [OUT]  (defaults 1M x 768, 8 queries, 5 rounds, profiles/r16_grouped.txt).

Data: tools/range_bench.py's (clustered Gaussians around 1 024 centres, rows normalised, fp32, L2 distance / Gaussian weights,
k = 25, topk = 15, tau = 0.62).  Cells: all N items with N/10 contiguous groups of 10, with 1 000 random labels and with 16
random labels; a prepared subset of N/10 uniformly random items with N/100 contiguous groups (by position in the subset); the
batched form, 256 queries over that subset.  n_groups = 10, per_group 1 and 3.  Every query's answer is checked against the
baseline's (labels, indices, score bits) before anything is timed; the checks are the warm-up."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import grouped_ref  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, make_queries, med  # noqa: E402

TAU = 0.62
NG = 10
BATCH = 256


def same(got, want):
    assert [(l, [i for i, _ in mem]) for l, mem in got] == [(l, [i for i, _ in mem]) for l, mem in want]
    assert np.array([v for _, mem in got for _, v in mem]).tobytes() == np.array([v for _, mem in want for _, v in mem]).tobytes()


def spread(x):
    return f"median {med(x):.1f} us (min {min(x):.1f}, max {max(x):.1f})"


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    nq = int(argv[2]) if len(argv) > 2 else 8
    rounds = int(argv[3]) if len(argv) > 3 else 5
    out = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "r16_grouped.txt")
    X = gpu_clustered(n, d, 42)
    gp = {"eps": calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = make_queries(X, max(nq, BATCH), 43)
    del X
    torch.cuda.synchronize()
    L = asp._L
    rng = np.random.default_rng(44)
    m_sub = max(n // 10, 1)
    some = np.sort(rng.choice(n, m_sub, replace=False))
    in_sub = np.zeros(n, dtype=np.int64)
    in_sub[some] = np.arange(m_sub) // 10
    cells = [(f"M=N={n}, {-(-n // 10)} contiguous groups of 10", None, np.arange(n) // 10),
             (f"M=N={n}, 1000 random labels", None, rng.integers(0, 1000, n)),
             (f"M=N={n}, 16 random labels", None, rng.integers(0, 16, n)),
             (f"M={m_sub}, {-(-m_sub // 10)} contiguous groups", some, in_sub)]
    lines = [f"search_grouped vs score_items + numpy group-by (grouped_ref): N={n} D={d} k=25 topk={gp['topk']} l2/gaussian "
             f"eps={gp['eps']:.5f} tau={TAU}, n_groups={NG}, {nq} queries x {rounds} rounds alternating; pick kernels = "
             f"group_pick_kernel launches by HIP events (separate pass); atomics = growth of as_grouped_counters[3] per call"]
    slower = []

    def timed_kernels(call):
        ks, at = [], []
        assert L.as_set_tuning(b"grouped_timing", 1) == 0
        try:
            for i in range(nq):
                c0 = aspace.grouped_counters()["max_atomics"]
                call(i)
                ks.append(L.as_grouped_kernel_us(aspace._h))
                at.append(aspace.grouped_counters()["max_atomics"] - c0)
        finally:
            assert L.as_set_tuning(b"grouped_timing", 0) == 0
        return ks, at

    for cname, ids, labels in cells:
        sub = None if ids is None else aspace.subset(ids)
        allsub = aspace.subset(np.arange(n)) if ids is None else sub
        ids = np.arange(n) if ids is None else ids
        lab_ids = labels[ids]
        grp = aspace.groups(labels)
        for pg in (1, 3):
            for i in range(nq):   # the answers, and the warm-up
                same(aspace.search_grouped(Q[i], gl, TAU, grp, NG, pg, subset=sub), grouped_ref.grouped(ids, lab_ids, aspace.score_items(Q[i], gl, TAU, ids), NG, pg))
                aspace.search_subset(Q[i], gl, TAU, allsub)
            t_new, t_old, t_sub = [], [], []
            for _ in range(rounds):
                for i in range(nq):
                    t0 = time.perf_counter()
                    aspace.search_grouped(Q[i], gl, TAU, grp, NG, pg, subset=sub)
                    t1 = time.perf_counter()
                    grouped_ref.grouped(ids, lab_ids, aspace.score_items(Q[i], gl, TAU, ids), NG, pg)
                    t2 = time.perf_counter()
                    aspace.search_subset(Q[i], gl, TAU, allsub)
                    t3 = time.perf_counter()
                    t_new.append((t1 - t0) * 1e6)
                    t_old.append((t2 - t1) * 1e6)
                    t_sub.append((t3 - t2) * 1e6)
            ks, at = timed_kernels(lambda i: aspace.search_grouped(Q[i], gl, TAU, grp, NG, pg, subset=sub))
            verdict = "" if med(t_new) <= med(t_old) else " -- SLOWER THAN THE BASELINE"
            if verdict:
                slower.append(f"{cname}, per_group={pg}")
            lines.append(f"{cname}, per_group={pg}: search_grouped {spread(t_new)} | baseline {spread(t_old)} | ratio {med(t_old) / med(t_new):.2f}x | "
                         f"search_subset over the same ids {spread(t_sub)} | grouped / search_subset {med(t_new) / med(t_sub):.2f} | pick kernels "
                         f"median {med(ks):.1f} us min {min(ks):.1f} us | max-atomics per call median {med(at):.0f} of {2 * pg * len(ids)} positions read{verdict}")
            print(lines[-1], flush=True)
        del grp, sub, allsub

    # the batched form over the subset
    cname, ids, labels = cells[3]
    sub, grp, lab_ids = aspace.subset(ids), aspace.groups(labels), labels[ids]
    QB = np.ascontiguousarray(Q[:BATCH])
    for pg in (1, 3):
        S = aspace.score_items_batch(QB, gl, TAU, ids)
        res = aspace.search_batch_grouped(QB, gl, TAU, grp, NG, pg, subset=sub)
        for i in range(BATCH):
            same(res[i], grouped_ref.grouped(ids, lab_ids, S[i], NG, pg))
        del S
        t_new, t_old = [], []
        for _ in range(rounds):
            t0 = time.perf_counter()
            aspace.search_batch_grouped(QB, gl, TAU, grp, NG, pg, subset=sub)
            t1 = time.perf_counter()
            S = aspace.score_items_batch(QB, gl, TAU, ids)
            for i in range(BATCH):
                grouped_ref.grouped(ids, lab_ids, S[i], NG, pg)
            t2 = time.perf_counter()
            t_new.append((t1 - t0) * 1e6)
            t_old.append((t2 - t1) * 1e6)
        assert L.as_set_tuning(b"grouped_timing", 1) == 0
        try:
            c0 = aspace.grouped_counters()["max_atomics"]
            aspace.search_batch_grouped(QB, gl, TAU, grp, NG, pg, subset=sub)
            ks, at = L.as_grouped_kernel_us(aspace._h), aspace.grouped_counters()["max_atomics"] - c0
        finally:
            assert L.as_set_tuning(b"grouped_timing", 0) == 0
        verdict = "" if med(t_new) <= med(t_old) else " -- SLOWER THAN THE BASELINE"
        if verdict:
            slower.append(f"B={BATCH} x {cname}, per_group={pg}")
        lines.append(f"B={BATCH} x {cname}, per_group={pg}: search_batch_grouped {spread(t_new)} | baseline {spread(t_old)} | ratio "
                     f"{med(t_old) / med(t_new):.2f}x | pick kernels {ks:.1f} us | max-atomics per call {at}{verdict}")
        print(lines[-1], flush=True)
    lines.append(f"grouped_counters {aspace.grouped_counters()}")
    lines.append("every cell at or below its baseline" if not slower else "cells slower than their baseline: " + "; ".join(slower))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
