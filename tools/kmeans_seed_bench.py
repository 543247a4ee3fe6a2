"""k-means++ seeding on the device at the headline size: what a step costs, where it goes, and whether
the seeding pays in Lloyd iterations.  python tools/kmeans_seed_bench.py [N] [D] [ROUNDS] [OUT]  (defaults 1M x 768, 3,
profiles/r28_kmeans_seed.txt).

Data and index: tools/range_bench.py's.  For k in {64, 1024} and L in {1, the default}: the whole `kmeans_seed` call by the wall
clock (median of ROUNDS) and per step; by HIP events ("kmeans_timing") the distance launches and the pick launches per step, the
distance kernel's bytes/s (the stored rows once, G read and written) next to `subset_score_kernel`'s over all N rows in the same
process, and the pick kernel's share of a step; one Lloyd iteration of the same k; then `kmeans(init="k-means++")` against
`kmeans(init=None)` on the same seed: iterations, final inertia, empty clusters and wall time.  Every line is written as measured,
the cells where the seeding does not pay included."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kmeans_seed_ref as ksr  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, med  # noqa: E402

L = asp._L
MAX_ITERS, SEED = 25, 0


def wall(call, rounds):
    call()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return med(ts)


def timed(aspace, call, entry, parts):
    """One call under "kmeans_timing" (after a warm-up) -> the parts `entry` reports."""
    assert L.as_set_tuning(b"kmeans_timing", 1) == 0
    try:
        call()
        call()
        return [entry(aspace._h, p) for p in range(parts)]
    finally:
        assert L.as_set_tuning(b"kmeans_timing", 0) == 0


def subset_tbs(aspace, gl, X, n, dp):
    """subset_score_kernel over all N rows, by HIP events -> TB/s."""
    sub = aspace.subset(np.arange(n))
    q = next(np.ascontiguousarray(X[i]) for i in range(n) if aspace.query_lambda(np.ascontiguousarray(X[i]), gl) != 0.0)
    aspace.search_subset(q, gl, 0.62, sub)
    sub.set_timing(True)
    ks = []
    for _ in range(8):
        aspace.search_subset(q, gl, 0.62, sub)
        ks.append(sub.kernel_us)
    sub.set_timing(False)
    return n * dp * 4 / (med(ks) * 1e-6) / 1e12


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    rounds = int(argv[2]) if len(argv) > 2 else 3
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r28_kmeans_seed.txt")
    Xd = gpu_clustered(n, d, 42)
    gp = {"eps": calibrate_eps(Xd, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, Xd.data_ptr(), "float32", n, d, d)
    torch.cuda.synchronize()
    X = Xd.cpu().numpy().astype(np.float64)
    dp = (d + 31) // 32 * 32
    lines = [f"kmeans_seed: N={n} D={d} fp32 rows; wall medians of {rounds}; seed {SEED}; kmeans max_iters = {MAX_ITERS}"]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(lines[-1], flush=True)

    flush()
    ref = subset_tbs(aspace, gl, X, n, dp)
    lines.append(f"subset_score_kernel over all {n} rows by HIP events: {ref:.2f} TB/s")
    flush()
    segs = (n + 255) // 256
    step_bytes = n * dp * 4 + 2 * segs * 256 * 16 * 8
    for k in (64, 1024):
        if k > n:
            continue
        us = timed(aspace, lambda: aspace.kmeans(k, seed=SEED, max_iters=2), L.as_kmeans_kernel_us, 4)
        lloyd = sum(us[:3]) / max(us[3], 1.0) / 1e3
        lines.append(f"k={k}: one Lloyd iteration (assign, ordering, update) by HIP events {lloyd:.2f} ms")
        flush()
        for trials in (1, None):
            Lr = trials or ksr.default_trials(k)
            ids, info = aspace.kmeans_seed(k, seed=SEED, trials=trials, with_info=True)
            assert len(set(ids.tolist())) == k and (np.diff(info["phi"]) <= 0).all() and info["degenerate"] == 0
            t = wall(lambda: aspace.kmeans_seed(k, seed=SEED, trials=trials), rounds)
            su = timed(aspace, lambda: aspace.kmeans_seed(k, seed=SEED, trials=trials), L.as_kmeans_seed_kernel_us, 3)
            dist_us, pick_us = su[0] / k, su[1] / k
            lines.append(f"k={k} L={Lr}: kmeans_seed {t:.1f} ms = {t / k * 1e3:.0f} us a pick = {t / lloyd:.1f} Lloyd iterations; by HIP events a step: "
                         f"distance kernel {dist_us:.0f} us = {step_bytes / 1e6:.0f} MB at {step_bytes / (dist_us * 1e-6) / 1e12:.2f} TB/s "
                         f"({step_bytes / (dist_us * 1e-6) / 1e12 / ref:.2f} of subset_score_kernel's), pick kernel {pick_us:.0f} us = "
                         f"{pick_us / (dist_us + pick_us):.2f} of the step; potential after the last pick {info['phi'][-1]:.6g}")
            flush()
        rows = []
        for init in (None, "k-means++"):
            t0 = time.perf_counter()
            _, _, info = aspace.kmeans(k, init=init, seed=SEED, max_iters=MAX_ITERS, with_info=True)
            rows.append((init, info, (time.perf_counter() - t0) * 1e3))
        for init, info, t in rows:
            lines.append(f"k={k} kmeans(init={init!r}): {info['iterations']} iterations, converged {info['converged']}, inertia {info['inertia']:.6f}, "
                         f"empty {info['empty']}, {t:.1f} ms with the seeding")
            flush()
    lines.append(f"kmeans_seed_counters {aspace.kmeans_seed_counters()}")
    flush()


if __name__ == "__main__":
    main()
