"""Bound-pruned spherical k-means at the headline size: `ArrowSpace.kmeans_spherical_bounded` against
`kmeans_spherical` -- the untouched path of the same build, never the new code -- from the same starting ids, the two alternating
in one process.
python tools/kmeans_spherical_bounded_bench.py [N] [D] [ROUNDS] [OUT]  (defaults 1M x 768, 5, profiles/r31_kmeans_spherical_bounded.txt).

Data, index and drawn ids: tools/kmeans_bounded_bench.py's.  First the answers are compared: labels, centroid bits, iterations,
changed counts and counts must be equal.  Then the active rows of every iteration, the wall clock of both calls (medians; the new
call wins where its median is below the baseline's by more than the larger of the two spreads), and by HIP events
("kmeans_timing") the shift, filter and assign launches of the bounded call next to the assign launches of `kmeans_spherical`."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyarrowspace_amd as asp  # noqa: E402
from kmeans_bounded_bench import MAX_ITERS, timed, verdict  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, med  # noqa: E402

L = asp._L


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    rounds = int(argv[2]) if len(argv) > 2 else 5
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r31_kmeans_spherical_bounded.txt")
    Xd = gpu_clustered(n, d, 42)
    gp = {"eps": calibrate_eps(Xd, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, Xd.data_ptr(), "float32", n, d, d)
    torch.cuda.synchronize()
    lines = [f"kmeans_spherical_bounded vs kmeans_spherical (the same build's untouched path): N={n} D={d} fp32 rows, init = the same k drawn "
             f"ids, max_iters = {MAX_ITERS}; {rounds} rounds alternating, medians"]
    print(lines[0], flush=True)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(lines[-1], flush=True)

    for k in (64, 1024):
        ids = np.random.default_rng(0).choice(n, k, replace=False)
        base = aspace.kmeans_spherical(k, init=ids, max_iters=MAX_ITERS, with_info=True)
        new = aspace.kmeans_spherical_bounded(k, init=ids, max_iters=MAX_ITERS, with_info=True)
        same = (np.array_equal(base[1], new[1]) and np.array_equal(base[0].view(np.uint64), new[0].view(np.uint64))
                and all(base[2][key] == new[2][key] for key in ("iterations", "converged", "changed", "empty")) and np.array_equal(base[2]["counts"], new[2]["counts"]))
        lines.append(f"k={k}: {new[2]['iterations']} iterations, converged {new[2]['converged']}; labels, centroid bits, changed and counts "
                     f"{'EQUAL' if same else 'DIFFER from'} kmeans_spherical's; cohesion {new[2]['cohesion']:.12g} (kmeans_spherical {base[2]['cohesion']:.12g})")
        lines.append(f"k={k} changed {new[2]['changed']}")
        lines.append(f"k={k} active  {new[2]['active']} = {sum(new[2]['active']) / (n * new[2]['iterations']):.3f} of the rows x iterations")
        flush()
        t_new, t_base = [], []
        for _ in range(rounds):
            t0 = time.perf_counter()
            aspace.kmeans_spherical(k, init=ids, max_iters=MAX_ITERS)
            t_base.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            aspace.kmeans_spherical_bounded(k, init=ids, max_iters=MAX_ITERS)
            t_new.append((time.perf_counter() - t0) * 1e6)
        lines.append(f"k={k} kmeans_spherical_bounded {med(t_new) / 1e3:.2f} ms [{min(t_new) / 1e3:.2f}, {max(t_new) / 1e3:.2f}] | kmeans_spherical "
                     f"{med(t_base) / 1e3:.2f} ms [{min(t_base) / 1e3:.2f}, {max(t_base) / 1e3:.2f}]: ratio {med(t_base) / med(t_new):.2f}x, {verdict(t_new, t_base)}")
        flush()
        ub = timed(aspace, lambda: aspace.kmeans_spherical_bounded(k, init=ids, max_iters=MAX_ITERS), L.as_kmeans_spherical_bounded_kernel_us)
        uk = timed(aspace, lambda: aspace.kmeans_spherical(k, init=ids, max_iters=MAX_ITERS), L.as_kmeans_spherical_kernel_us)
        its = max(ub[3], 1.0)
        lines.append(f"k={k} by HIP events over {int(its)} iterations: shift {ub[0]:.0f} us, filter {ub[1]:.0f} us ({ub[1] / max(its - 1, 1):.0f} us a pass = "
                     f"{n * d * 4 / max(ub[1] / max(its - 1, 1), 1e-9) / 1e6:.2f} TB/s of row bytes), assign {ub[2]:.0f} us | kmeans_spherical's assign launches {uk[1]:.0f} us")
        flush()
    lines.append(f"kmeans_spherical_bounded_counters {aspace.kmeans_spherical_bounded_counters()}")
    flush()


if __name__ == "__main__":
    main()
