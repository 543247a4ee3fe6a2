"""Batched filtered search at the headline size: `search_batch_subset` over one prepared subset of M items for B queries, against
the per-query median of `search_subset` that tools/subset_bench.py recorded for the same M (profiles/r08_subset.txt).
python tools/subset_batch_bench.py [N] [D] [OUT]  (defaults 1M x 768, profiles/r09_subset_batch.txt).

Data, queries, parameters and subsets are those of tools/subset_bench.py (clustered Gaussians by the torch RNG, seed 42; L2 /
Gaussian, k = 25, topk = 15, tau = 0.62; bench.make_queries, seed 43; M = 1 000 and 100 000 uniformly random items, seed 44, and
all N).  Grid: M x B in {32, 256, 1024}.  Every cell's lists are checked first against a loop of `search_subset` (all of the
first 32 queries and the last 8) with `same_as_single`.  Per cell: median wall time of a call and per query, the `search_batch`
call alone (lambda_q comes from it), the batched score kernel's device time by HIP events (summed over the call's chunks), and
the fp64 MFMA FLOP/s it issued -- 2 x M_padded x B_padded x dp per unit of kernel time, M padded to the 128-row tile and B to
the 64-query tile -- as a fraction of bench.py's MFMA_F64_PEAK_TF (gram_f64_kernel, the project's other fp64 MFMA kernel,
reaches 0.57 of it)."""
import os
import re
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

GRAM_FRACTION = 0.57
ROW_TILE, QUERY_TILE = 128, 64
BS = (32, 256, 1024)
REPS = 5


def single_medians(path):
    """M -> the per-query median of search_subset in tools/subset_bench.py's profile (microseconds); {} without the file."""
    out = {}
    if os.path.exists(path):
        for line in open(path):
            m = re.match(r"M=(\d+): .*search_subset median ([0-9.]+) us", line)
            if m:
                out[int(m.group(1))] = float(m.group(2))
    return out


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    out = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "r09_subset_batch.txt")
    single = single_medians(os.path.join(ROOT, "profiles", "r08_subset.txt"))
    peak = bench.MFMA_F64_PEAK_TF
    X = gpu_clustered(n, d, 42)
    gp = {"eps": bench.calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = np.ascontiguousarray(np.stack([np.ascontiguousarray(q) for q in bench.make_queries(X, max(BS), 43)]))
    del X
    torch.cuda.synchronize()
    dp = (d + 31) // 32 * 32
    tau = 0.62
    rng = np.random.default_rng(44)
    lines = [f"search_batch_subset: N={n} D={d} k=25 topk=15 l2/gaussian eps={gp['eps']:.5f} tau={tau}, one prepared subset per M, median of "
             f"{REPS} calls per cell; kernel = subset_score_batch_kernel by HIP events, summed over the chunks of a call; MFMA fraction = "
             f"2 x M_padded x B_padded x {dp} / kernel time / {peak} TFLOP/s (gram_f64_kernel: {GRAM_FRACTION}); single = search_subset's "
             f"per-query median for the same M in profiles/r08_subset.txt"]
    worse = []
    for m in sorted({min(1_000, n), min(100_000, n), n}):
        ids = np.arange(n) if m == n else np.sort(rng.choice(n, m, replace=False))
        sub = aspace.subset(ids)
        for b in BS:
            Qb = np.ascontiguousarray(Q[:b])
            got = aspace.search_batch_subset(Qb, gl, tau, sub)   # warm-up (the batched buffers are made here), and the lists
            for i in list(range(min(b, 32))) + list(range(max(b - 8, 32), b)):
                same_as_single(got[i], aspace.search_subset(np.ascontiguousarray(Qb[i]), gl, tau, sub))
            sub.set_timing(True)
            t_call, t_sb, ks = [], [], []
            for _ in range(REPS):
                t0 = time.perf_counter()
                aspace.search_batch(Qb, gl, tau)
                t1 = time.perf_counter()
                aspace.search_batch_subset(Qb, gl, tau, sub)
                t2 = time.perf_counter()
                t_sb.append((t1 - t0) * 1e6)
                t_call.append((t2 - t1) * 1e6)
                ks.append(sub.kernel_us)
            sub.set_timing(False)
            call, sb, ku = float(np.median(t_call)), float(np.median(t_sb)), float(np.median(ks))
            mp, bp = (m + ROW_TILE - 1) // ROW_TILE * ROW_TILE, (b + QUERY_TILE - 1) // QUERY_TILE * QUERY_TILE
            frac = 2.0 * mp * bp * dp / (ku * 1e-6) / 1e12 / peak
            ref = single.get(m)
            if ref is None:
                verdict = "single: no profile"
            else:
                verdict = f"single {ref:.1f} us/query: {'below it' if call / b < ref else 'NOT BELOW IT'} ({ref / (call / b):.1f}x)"
                if not call / b < ref:
                    worse.append((m, b))
            lines.append(f"M={m} B={b}: call {call:.0f} us = {call / b:.1f} us/query | search_batch alone {sb:.0f} us = {sb / b:.1f} us/query | "
                         f"score kernel {ku:.0f} us, {2.0 * mp * bp * dp / 1e9:.1f} GFLOP issued = {frac:.2f} of the fp64 MFMA peak "
                         f"({frac / GRAM_FRACTION:.2f} of gram_f64_kernel's fraction) | {verdict}")
            print(lines[-1], flush=True)
        del sub
    lines.append("cells not below the single form's per-query median: " + (", ".join(f"M={m} B={b}" for m, b in worse) if worse else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
