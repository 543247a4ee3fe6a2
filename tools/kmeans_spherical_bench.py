"""Spherical k-means over the items at the headline size: `ArrowSpace.assign_cosine` against `assign`
and `kmeans_spherical` against `kmeans` of the same build, alternating in one process.
python tools/kmeans_spherical_bench.py [N] [D] [ROUNDS] [OUT]  (defaults 1M x 768, 5, profiles/r30_kmeans_spherical.txt).

Data and index: tools/range_bench.py's.  The answer is checked first, on a row sample, by the rule of
tests/test_gpu_kmeans_spherical.py (cos within E of the longdouble cosine, the label inside the near-tie set).  Criterion for the
assignment: `assign_cosine`'s median does not exceed `assign`'s by more than the larger of the two spreads.  Then by HIP events
("kmeans_timing"): the unit, assign, ordering and update launches per iteration beside `kmeans`'s, and the assign kernel's
fraction of the fp64 MFMA peak (78.6 TFLOP/s, as profiles/r27_kmeans.txt)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kmeans_spherical_ref as ks  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, med  # noqa: E402

L = asp._L
PEAK, LLOYD_ITERS = 78.6e12, 3


def span(ts):
    return f"{med(ts) / 1e3:.2f} ms [{min(ts) / 1e3:.2f}, {max(ts) / 1e3:.2f}]"


def alternate(rounds, a, b):
    ta, tb = [], []
    for _ in range(rounds):
        for call, ts in ((a, ta), (b, tb)):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e6)
    return ta, tb


def timed(aspace, call, parts, nparts):
    """One call under "kmeans_timing" (after a warm-up) -> the microseconds of `parts`."""
    assert L.as_set_tuning(b"kmeans_timing", 1) == 0
    try:
        call()
        call()
        return [parts(aspace._h, p) for p in range(nparts)]
    finally:
        assert L.as_set_tuning(b"kmeans_timing", 0) == 0


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    rounds = int(argv[2]) if len(argv) > 2 else 5
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r30_kmeans_spherical.txt")
    Xd = gpu_clustered(n, d, 42)
    gp = {"eps": calibrate_eps(Xd, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, Xd.data_ptr(), "float32", n, d, d)
    torch.cuda.synchronize()
    sample = np.sort(np.random.default_rng(3).choice(n, min(n, 2048), replace=False))
    Xs = Xd[torch.as_tensor(sample, device=Xd.device)].cpu().numpy().astype(np.float64)
    lines = [f"assign_cosine vs assign, kmeans_spherical vs kmeans: N={n} D={d} fp32 rows; {rounds} rounds alternating, median [min, max]; "
             f"Lloyd: init = the seed's rows, max_iters = {LLOYD_ITERS} on both sides"]
    print(lines[0], flush=True)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(lines[-1], flush=True)

    for k in (64, 1024):
        ids = np.random.default_rng(0).choice(n, k, replace=False)
        C = np.stack([aspace.get_item(int(i))[0] for i in ids])
        labels, cos = aspace.assign_cosine(C, with_cos=True)
        G, at = ks.cosines(Xs, C), np.arange(len(sample))
        err = float(np.abs(cos[sample] - G[at, labels[sample]]).max())
        assert err <= ks.E(d) and (G[at, labels[sample]] >= G.max(axis=1) - 2.0 * ks.E(d)).all()
        moved = int((labels != aspace.assign(C)).sum())
        lines.append(f"k={k}: {len(sample)} sampled rows pass the near-tie rule, cos within {err:.3g} of the longdouble cosine (E = {ks.E(d):.3g}); "
                     f"{moved} of {n} items carry another label than under assign (squared L2)")
        flush()
        t_cos, t_l2 = alternate(rounds, lambda: aspace.assign_cosine(C, with_cos=True), lambda: aspace.assign(C, with_dist=True))
        spread = max(max(t_cos) - min(t_cos), max(t_l2) - min(t_l2))
        ok = med(t_cos) <= med(t_l2) + spread
        lines.append(f"k={k} assign_cosine {span(t_cos)} | assign {span(t_l2)}: assign_cosine's median "
                     f"{'does not exceed' if ok else 'EXCEEDS'} assign's by more than the larger spread ({spread / 1e3:.2f} ms)")
        flush()
        us = timed(aspace, lambda: aspace.assign_cosine(C), L.as_kmeans_spherical_kernel_us, 5)
        ul = timed(aspace, lambda: aspace.assign(C), L.as_kmeans_kernel_us, 4)
        kp, dp, npad = (k + 63) // 64 * 64, (d + 31) // 32 * 32, (n + 127) // 128 * 128
        flops = 2.0 * npad * kp * dp
        lines.append(f"k={k} by HIP events: unit {us[0]:.1f} us, kms_assign_kernel {us[1] / 1e3:.2f} ms = {flops / (us[1] * 1e-6) / PEAK:.2f} of the fp64 "
                     f"MFMA peak | assign's norms + km_assign_kernel {ul[0] / 1e3:.2f} ms = {flops / (ul[0] * 1e-6) / PEAK:.2f}")
        flush()
        cent, lab, info = aspace.kmeans_spherical(k, init=ids, max_iters=LLOYD_ITERS, with_info=True)
        lines.append(f"k={k} kmeans_spherical: {info['iterations']} iterations, changed {info['changed']}, empty {info['empty']}, cohesion "
                     f"{info['cohesion']:.6f}; the centroids' squared lengths lie within {float(np.abs((cent * cent).sum(axis=1) - 1).max()):.3g} of 1")
        flush()
        t_sph, t_km = alternate(rounds, lambda: aspace.kmeans_spherical(k, init=ids, max_iters=LLOYD_ITERS),
                                lambda: aspace.kmeans(k, init=ids, max_iters=LLOYD_ITERS))
        lines.append(f"k={k} kmeans_spherical {span(t_sph)} | kmeans {span(t_km)}, {LLOYD_ITERS} iterations each: per iteration "
                     f"{med(t_sph) / LLOYD_ITERS / 1e3:.2f} ms | {med(t_km) / LLOYD_ITERS / 1e3:.2f} ms")
        flush()
        us = timed(aspace, lambda: aspace.kmeans_spherical(k, init=ids, max_iters=LLOYD_ITERS), L.as_kmeans_spherical_kernel_us, 5)
        ul = timed(aspace, lambda: aspace.kmeans(k, init=ids, max_iters=LLOYD_ITERS), L.as_kmeans_kernel_us, 4)
        its, itl = max(us[4], 1.0), max(ul[3], 1.0)
        lines.append(f"k={k} per iteration by HIP events: kmeans_spherical unit {us[0] / its:.1f} us, assign {us[1] / its / 1e3:.2f} ms, ordering "
                     f"{us[2] / its:.1f} us, update (segment sums, final) {us[3] / its:.1f} us | kmeans assign {ul[0] / itl / 1e3:.2f} ms, ordering "
                     f"{ul[1] / itl:.1f} us, update {ul[2] / itl:.1f} us")
        flush()
    lines.append(f"kmeans_spherical_counters {aspace.kmeans_spherical_counters()}")
    flush()


if __name__ == "__main__":
    main()
