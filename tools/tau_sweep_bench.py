"""Tau sweeps at the headline size: one `search_taus` call against the T single searches it replaces, per query, alternating
in one process.  python tools/tau_sweep_bench.py [N] [D] [NQ] [OUT] [--sweep-only]  (defaults 1M x 768, 64 queries,
profiles/r06_tau_sweep.txt).  --sweep-only: the search_taus calls alone, no check and no single searches (the kernel list of
a sweep under `rocprofv3 --kernel-trace --stats`, profiles/r06_tau_sweep_kernels.csv).

Data: the clustered-Gaussian recipe of tests/conftest.py::gpu_clustered (torch RNG, seed 42), L2 distance / Gaussian weights,
k = 25, topk = 15, eps calibrated as bench.py does; queries: bench.make_queries (perturbed items, seed 43).  Every sweep's
lists are checked against the single searches before timing.  Reports median / p90 microseconds per query of both forms,
their ratio and the space's sweep_counters()."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402

TAU_SETS = [("scripts' triple", [1.0, 0.8, 0.62]), ("BEIR sweep", [0.62, 0.8, 0.42, 0.0]), ("six spread", [1.0, 0.8, 0.6, 0.4, 0.2, 0.0])]


def gpu_clustered(n, d, seed, nclust=1024, noise=0.5, device="cuda"):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    C = torch.randn((nclust, d), generator=g, device=device, dtype=torch.float32)
    z = torch.randint(0, nclust, (n,), generator=g, device=device)
    X = torch.empty((n, d), device=device, dtype=torch.float32)
    for s in range(0, n, 1 << 17):
        e = min(n, s + (1 << 17))
        X[s:e] = C[z[s:e]] + noise * torch.randn((e - s, d), generator=g, device=device, dtype=torch.float32)
        X[s:e] /= X[s:e].norm(dim=1, keepdim=True)
    return X


def main():
    sweep_only = "--sweep-only" in sys.argv
    argv = [a for a in sys.argv[1:] if a != "--sweep-only"]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    nq = int(argv[2]) if len(argv) > 2 else 64
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r06_tau_sweep.txt")
    X = gpu_clustered(n, d, 42)
    gp = {"eps": bench.calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = [np.ascontiguousarray(q) for q in bench.make_queries(X, nq, 43)]
    del X
    torch.cuda.synchronize()
    if sweep_only:
        for name, taus in TAU_SETS:
            for q in Q:
                aspace.search_taus(q, gl, taus)
        print("sweep_counters", aspace.sweep_counters())
        return
    lines = [f"tau sweep vs single searches: N={n} D={d} k=25 topk=15 l2/gaussian eps={gp['eps']:.5f}, {nq} queries, B=1"]
    for name, taus in TAU_SETS:
        for q in Q[:8]:   # warm-up, and the lists against the single searches (exact scores: the same bits)
            got = aspace.search_taus(q, gl, taus)
            for j, t in enumerate(taus):
                want = aspace.search(q, gl, t)
                assert [i for i, _ in got[j]] == [i for i, _ in want], (name, t)
                np.testing.assert_allclose([s for _, s in got[j]], [s for _, s in want], rtol=1e-12, atol=0.0)
        c0 = aspace.sweep_counters()
        ts_single, ts_sweep = [], []
        for r in range(3):
            for q in Q:
                t0 = time.perf_counter()
                for t in taus:
                    aspace.search(q, gl, t)
                t1 = time.perf_counter()
                aspace.search_taus(q, gl, taus)
                t2 = time.perf_counter()
                ts_single.append((t1 - t0) * 1e6)
                ts_sweep.append((t2 - t1) * 1e6)
        c1 = aspace.sweep_counters()
        m1, m2 = float(np.median(ts_single)), float(np.median(ts_sweep))
        p1, p2 = float(np.percentile(ts_single, 90)), float(np.percentile(ts_sweep, 90))
        dc = {k: c1[k] - c0[k] for k in c1}
        lines.append(f"{name} {taus}: {len(taus)} single searches median {m1:.1f} us p90 {p1:.1f} us | search_taus median {m2:.1f} us "
                     f"p90 {p2:.1f} us | ratio {m2 / m1:.3f} | counters over the timed calls {dc}")
        print(lines[-1], flush=True)
    lines.append(f"search_counters {aspace.search_counters()}  sweep_counters {aspace.sweep_counters()}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
