"""Batched tau sweeps: one `search_batch_taus` call against the T back-to-back `search_batch` calls it replaces.
python tools/batch_sweep_bench.py [N] [D] [B] [taus...] [--sweep-only]  (defaults 1M x 768, B = 1024, taus 1 .8 .62).
--sweep-only: two `search_batch_taus` calls alone, no check and no timing (the kernel list of a sweep under
`rocprofv3 --kernel-trace --stats`).

Data: the clustered-Gaussian recipe of tools/tau_sweep_bench.py (torch RNG, seed 42), L2 distance / Gaussian weights,
k = 25, topk = 15, eps calibrated as bench.py does; queries: bench.make_queries (perturbed items, seed 43).  First the
sweep's lists are checked against search_batch per tau on sampled slots ([b][j] == search_batch(Q, gl, taus[j])[b]); then
the two forms are timed alternately, 5 rounds, and the medians, their ratio and batch_sweep_counters() are printed."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from tau_sweep_bench import gpu_clustered  # noqa: E402


def main():
    sweep_only = "--sweep-only" in sys.argv
    argv = [a for a in sys.argv[1:] if a != "--sweep-only"]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    b = int(argv[2]) if len(argv) > 2 else 1024
    taus = [float(t) for t in argv[3:]] or [1.0, 0.8, 0.62]
    X = gpu_clustered(n, d, 42)
    gp = {"eps": bench.calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = np.ascontiguousarray(np.stack([np.asarray(q) for q in bench.make_queries(X, b, 43)]))
    del X
    torch.cuda.synchronize()
    if sweep_only:
        for _ in range(2):
            aspace.search_batch_taus(Q, gl, taus)
        print("batch_sweep_counters", aspace.batch_sweep_counters())
        return
    got = aspace.search_batch_taus(Q, gl, taus)
    rows = range(0, b, max(1, b // 64))
    for j, t in enumerate(taus):
        want = aspace.search_batch(Q, gl, t)
        for r in rows:
            assert got[r][j] == want[r], (r, t)
    c0 = aspace.batch_sweep_counters()
    ts_batch, ts_sweep = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        for t in taus:
            aspace.search_batch(Q, gl, t)
        t1 = time.perf_counter()
        aspace.search_batch_taus(Q, gl, taus)
        t2 = time.perf_counter()
        ts_batch.append((t1 - t0) * 1e3)
        ts_sweep.append((t2 - t1) * 1e3)
    c1 = aspace.batch_sweep_counters()
    m1, m2 = float(np.median(ts_batch)), float(np.median(ts_sweep))
    dc = {k: c1[k] - c0[k] for k in c1}
    print(f"N={n} D={d} B={b} T={len(taus)} taus {taus}: {len(taus)} x search_batch median {m1:.1f} ms | search_batch_taus median "
          f"{m2:.1f} ms | ratio {m2 / m1:.3f} | {b * len(taus) / m2 * 1e3:.0f} (query, tau) pairs/s | counters over the timed calls {dc}",
          flush=True)


if __name__ == "__main__":
    main()
