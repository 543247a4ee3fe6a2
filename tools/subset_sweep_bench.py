"""Tau sweeps over a subset at the headline size: `search_subset_taus` (B = 1) and `search_batch_subset_taus` (B = 1024) over one
prepared subset of M items, against T back-to-back calls of the unchanged single-tau form (`search_subset`, `search_batch_subset`)
in the same process.  python tools/subset_sweep_bench.py [N] [D] [OUT]  (defaults 1M x 768, profiles/r10_subset_sweep.txt).

Data, queries, parameters and subsets are those of tools/subset_bench.py (clustered Gaussians by the torch RNG, seed 42; L2 /
Gaussian, k = 25, topk = 15, fp32 rows; bench.make_queries, seed 43; M = 1 000 and 100 000 uniformly random items, seed 44, and
all N).  Tau sets: {1, .8, .62} and {1, .8, .62, .42, .2, 0}.  Every cell's lists are checked first against the loop of single-tau
calls with `same_as_single`.  Then, after a warm-up of both, sweep and loop alternate REPS times; a cell reports the two medians
of the wall time of a call (each call ends in a stream wait), their ratio, and the device time of the score kernels by HIP events
(`as_subset_kernel_us`): the sweep's kernel, summed over the call's launches, beside the single-tau kernel summed over the loop's
T calls.  The sweep replaces T - 1 lambda_q steps and T - 1 gathers by T - 1 extra store planes; where one gather serves all T taus the
extra planes cost the difference between the sweep's kernel time and ONE single-tau kernel's.  B = 1 cells time REPS_SINGLE queries in turn."""
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

TAU_SETS = ((1.0, 0.8, 0.62), (1.0, 0.8, 0.62, 0.42, 0.2, 0.0))
B_BATCH = 1024
REPS_SINGLE, REPS_BATCH = 40, 7


def cell(sweep, loop, sub, reps, args):
    """alternating: medians of the call times (us) and of the score kernels' device times"""
    for a in args[:2]:
        sweep(a)
        loop(a)
    sub.set_timing(True)
    ts, tl, ks, kl = [], [], [], []
    for r in range(reps):
        a = args[r % len(args)]
        t0 = time.perf_counter()
        sweep(a)
        t1 = time.perf_counter()
        ks.append(sub.kernel_us)
        t2 = time.perf_counter()
        kl.append(loop(a, kernel=True))
        t3 = time.perf_counter()
        ts.append((t1 - t0) * 1e6)
        tl.append((t3 - t2) * 1e6)
    sub.set_timing(False)
    return float(np.median(ts)), float(np.median(tl)), float(np.median(ks)), float(np.median(kl))


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    out = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "r10_subset_sweep.txt")
    X = gpu_clustered(n, d, 42)
    gp = {"eps": bench.calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = np.ascontiguousarray(np.stack([np.ascontiguousarray(q) for q in bench.make_queries(X, B_BATCH, 43)]))
    del X
    torch.cuda.synchronize()
    rng = np.random.default_rng(44)
    lines = [f"tau sweeps over a subset: N={n} D={d} k=25 topk=15 l2/gaussian eps={gp['eps']:.5f}, one prepared subset per M; sweep and "
             f"loop of T single-tau calls alternate in one process, medians of {REPS_SINGLE} (B=1) / {REPS_BATCH} (B={B_BATCH}) calls; "
             f"kernel = the score kernels' device time by HIP events (sweep: summed over the call's launches; loop: summed over its T calls)"]
    worse = []
    for m in sorted({min(1_000, n), min(100_000, n), n}):
        ids = np.arange(n) if m == n else np.sort(rng.choice(n, m, replace=False))
        sub = aspace.subset(ids)
        for taus in TAU_SETS:
            nt = len(taus)
            for b in (1, B_BATCH):
                if b == 1:
                    args = [np.ascontiguousarray(Q[i]) for i in range(REPS_SINGLE)]

                    def sweep(q):
                        return aspace.search_subset_taus(q, gl, taus, sub)

                    def loop(q, kernel=False):
                        k, res = 0.0, []
                        for tau in taus:
                            res.append(aspace.search_subset(q, gl, tau, sub))
                            k += sub.kernel_us if kernel else 0.0
                        return k if kernel else res

                    for q in args[:8]:
                        for got, want in zip(sweep(q), loop(q)):
                            same_as_single(got, want)
                    reps = REPS_SINGLE
                else:
                    args = [np.ascontiguousarray(Q[:b])]

                    def sweep(Qb):
                        return aspace.search_batch_subset_taus(Qb, gl, taus, sub)

                    def loop(Qb, kernel=False):
                        k, res = 0.0, []
                        for tau in taus:
                            res.append(aspace.search_batch_subset(Qb, gl, tau, sub))
                            k += sub.kernel_us if kernel else 0.0
                        return k if kernel else res

                    got, want = sweep(args[0]), loop(args[0])
                    for i in list(range(32)) + list(range(b - 8, b)):
                        for j in range(nt):
                            same_as_single(got[i][j], want[j][i])
                    reps = REPS_BATCH
                ts, tl, ks, kl = cell(sweep, loop, sub, reps, args)
                below = ts < tl
                if not below:
                    worse.append((m, nt, b))
                lines.append(f"M={m} T={nt} B={b}: sweep {ts:.0f} us = {ts / b:.1f} us/query | loop of {nt} single-tau calls {tl:.0f} us = "
                             f"{tl / b:.1f} us/query | ratio {tl / ts:.2f}x, {'below the loop' if below else 'NOT BELOW THE LOOP'} | score kernels: "
                             f"sweep {ks:.0f} us, loop {kl:.0f} us = {kl / nt:.0f} us a call; sweep minus one single-tau kernel "
                             f"{ks - kl / nt:.0f} us")
                print(lines[-1], flush=True)
        del sub
    lines.append("cells where the sweep's median is not below the loop's: " +
                 (", ".join(f"M={m} T={t} B={b}" for m, t, b in worse) if worse else "none"))
    lines.append(f"subset_sweep_counters: {aspace.subset_sweep_counters()}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
