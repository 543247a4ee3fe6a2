"""Filtered search at the headline size: `search_subset` over one prepared subset of M items against `search` alone, per query,
alternating in one process, and the score kernel's own duration by HIP events.
python tools/subset_bench.py [N] [D] [NQ] [OUT]  (defaults 1M x 768, 64 queries, profiles/r08_subset.txt).

Data: the clustered-Gaussian recipe of tests/conftest.py::gpu_clustered (torch RNG, seed 42), L2 distance / Gaussian weights,
k = 25, topk = 15, eps calibrated as bench.py does; queries: bench.make_queries (perturbed items, seed 43).  Subsets: M = 1 000
and 100 000 uniformly random items, and all N.  Every subset's lists are checked before timing: M = N against `search`, the
others against numpy over `score_items` of the subset's ids.  Reports median / p90 microseconds per query of both calls, the
kernel's median microseconds, and its gathered bytes (M x dp x 4: fp32 rows) per second against the guide's rate for whole rows
gathered into registers (5.5 TB/s, measured there for rows of 1-2 KB; 3 KB rows are not in that table)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from tau_sweep_bench import gpu_clustered  # noqa: E402

YARDSTICK_TBS = 5.5


def same_as_single(got, single, tie=1e-12):
    """What the library promises for the full subset: search's indices in search's order except where two scores tie to
    `tie` relative, scores within `tie` relative."""
    assert len(got) == len(single), (got, single)
    ws = np.array([s for _, s in single])
    np.testing.assert_allclose([s for _, s in got], ws, rtol=tie, atol=0.0)
    for t, ((a, _), (b, _)) in enumerate(zip(got, single)):
        if a != b:
            tied = [single[u][0] for u in range(len(ws)) if abs(ws[u] - ws[t]) <= tie * max(abs(ws[t]), 1e-300)]
            assert len(tied) > 1 and a in tied, (t, got, single)


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    nq = int(argv[2]) if len(argv) > 2 else 64
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r08_subset.txt")
    X = gpu_clustered(n, d, 42)
    gp = {"eps": bench.calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = [np.ascontiguousarray(q) for q in bench.make_queries(X, nq, 43)]
    del X
    torch.cuda.synchronize()
    dp = (d + 31) // 32 * 32
    tau = 0.62
    rng = np.random.default_rng(44)
    lines = [f"search_subset vs search: N={n} D={d} k=25 topk=15 l2/gaussian eps={gp['eps']:.5f} tau={tau}, {nq} queries, B=1, one prepared "
             f"subset per M; kernel = subset_score_kernel by HIP events; yardstick {YARDSTICK_TBS} TB/s (whole rows gathered into registers)"]
    for m in sorted({min(1_000, n), min(100_000, n), n}):
        ids = np.arange(n) if m == n else np.sort(rng.choice(n, m, replace=False))
        sub = aspace.subset(ids)
        for q in Q[:4]:   # warm-up, and the lists
            got = aspace.search_subset(q, gl, tau, sub)
            if m == n:
                want = aspace.search(q, gl, tau)
                same_as_single(got, want)
            else:
                sc = aspace.score_items(q, gl, tau, ids)
                order = np.lexsort((ids, -sc))[:len(got)]
                assert [i for i, _ in got] == ids[order].tolist(), (m, got)
                assert [s for _, s in got] == sc[order].tolist(), (m, got)
        sub.set_timing(True)
        ts_single, ts_sub, ks = [], [], []
        for r in range(3):
            for q in Q:
                t0 = time.perf_counter()
                aspace.search(q, gl, tau)
                t1 = time.perf_counter()
                aspace.search_subset(q, gl, tau, sub)
                t2 = time.perf_counter()
                ts_single.append((t1 - t0) * 1e6)
                ts_sub.append((t2 - t1) * 1e6)
                ks.append(sub.kernel_us)
        sub.set_timing(False)
        m1, m2, mk = float(np.median(ts_single)), float(np.median(ts_sub)), float(np.median(ks))
        p1, p2 = float(np.percentile(ts_single, 90)), float(np.percentile(ts_sub, 90))
        tbs = m * dp * 4 / (mk * 1e-6) / 1e12
        verdict = "" if tbs >= YARDSTICK_TBS / 2 else " -- LESS THAN HALF the yardstick"
        lines.append(f"M={m}: search median {m1:.1f} us p90 {p1:.1f} us | search_subset median {m2:.1f} us p90 {p2:.1f} us | beside search "
                     f"+{m2 - m1:.1f} us | kernel median {mk:.1f} us min {min(ks):.1f} us, {m * dp * 4 / 1e6:.1f} MB gathered = {tbs:.2f} TB/s "
                     f"({tbs / YARDSTICK_TBS:.2f} of the yardstick){verdict}")
        print(lines[-1], flush=True)
        del sub
    lines.append(f"search_counters {aspace.search_counters()}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
