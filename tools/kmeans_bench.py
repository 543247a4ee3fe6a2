"""k-means over the items at the headline size: `ArrowSpace.assign` and `kmeans` against the routes
there were before -- a host float64 GEMM-argmin over the items in row chunks (numpy), `score_items_batch` over all ids for one
tile of centroids (stated per centroid), and for `kmeans` the same host loop with tests/kmeans_ref.py's update -- the routes
alternating in one process.  python tools/kmeans_bench.py [N] [D] [ROUNDS] [OUT]  (defaults 1M x 768, 5, profiles/r27_kmeans.txt).

Data and index: tools/range_bench.py's.  Every answer is checked first: the labels against the host route's, and wherever the two
differ -- and on a row sample by direct differences -- by the rule of tests/test_gpu_kmeans.py (dist within E, the label inside the
near-tie set).  Criterion, the project's own: the new call's median is below the baseline's by more than the baseline's own
spread.  Then by HIP events ("kmeans_timing"): the assign, ordering and update launches, the assign kernel's fraction of the fp64
MFMA peak (78.6 TFLOP/s, as profiles/r09_subset_batch.txt) and the bytes the update moves."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kmeans_ref as kr  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from components_bench import verdict  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, med  # noqa: E402

L = asp._L
CHUNK, PEAK, HBM, LLOYD_ITERS = 65536, 78.6e12, 8e12, 2


def host_assign(X, nx, C):
    """labels, dist by the norm expansion, float64, in row chunks: the k x N matrix never exists as a whole."""
    cn = (C * C).sum(axis=1)
    labels, dist = np.empty(X.shape[0], dtype=np.int32), np.empty(X.shape[0])
    for s in range(0, X.shape[0], CHUNK):
        key = cn[None, :] - 2.0 * (X[s:s + CHUNK] @ C.T)
        j = key.argmin(axis=1)
        labels[s:s + CHUNK] = j
        dist[s:s + CHUNK] = np.maximum(nx[s:s + CHUNK] + key[np.arange(len(j)), j], 0.0)
    return labels, dist


def host_kmeans(X, nx, C, iters):
    prev = None
    for _ in range(iters):
        labels, _ = host_assign(X, nx, C)
        if prev is not None and np.array_equal(labels, prev):
            break
        C, prev = kr.update(X, labels, C), labels
    return C, labels


def check(X, C, labels, dist, rows):
    D, E = kr.dists(X[rows], C), kr.bound(X[rows], C)
    at = np.arange(len(rows))
    assert (np.abs(dist[rows] - D[at, labels[rows]]) <= E[at, labels[rows]]).all()
    assert (D[at, labels[rows]] <= D.min(axis=1) + 2.0 * E.max(axis=1)).all()


def timed(aspace, call):
    """One call under "kmeans_timing" (after a warm-up) -> as_kmeans_kernel_us's parts."""
    assert L.as_set_tuning(b"kmeans_timing", 1) == 0
    try:
        call()
        call()
        return [L.as_kmeans_kernel_us(aspace._h, p) for p in range(4)]
    finally:
        assert L.as_set_tuning(b"kmeans_timing", 0) == 0


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    rounds = int(argv[2]) if len(argv) > 2 else 5
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r27_kmeans.txt")
    Xd = gpu_clustered(n, d, 42)
    eps = calibrate_eps(Xd, 25)
    gp = {"eps": eps, "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, Xd.data_ptr(), "float32", n, d, d)
    torch.cuda.synchronize()
    X = Xd.cpu().numpy().astype(np.float64)
    nx = np.einsum("ij,ij->i", X, X)
    lines = [f"assign / kmeans vs a host float64 GEMM-argmin in chunks of {CHUNK} rows (numpy, {os.cpu_count()} CPUs visible): N={n} D={d} fp32 rows; "
             f"{rounds} rounds alternating, medians; kmeans: init = the seed's rows, max_iters = {LLOYD_ITERS} on both sides"]
    print(lines[0], flush=True)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(lines[-1], flush=True)

    rng = np.random.default_rng(3)
    sample = np.sort(rng.choice(n, min(n, 2048), replace=False))
    for k in (64, 1024):
        ids = np.random.default_rng(0).choice(n, k, replace=False)
        C = X[ids]
        labels, dist = aspace.assign(C, with_dist=True)
        want, _ = host_assign(X, nx, C)
        differ = np.flatnonzero(labels != want)
        check(X, C, labels, dist, np.union1d(sample, differ[:4096]))
        lines.append(f"k={k}: the labels differ from the host route's at {len(differ)} of {n} items; those and {len(sample)} sampled rows pass the "
                     f"near-tie rule and the dist bound against direct differences")
        flush()
        t_new, t_old = [], []
        for _ in range(rounds):
            t0 = time.perf_counter()
            aspace.assign(C, with_dist=True)
            t_new.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            host_assign(X, nx, C)
            t_old.append((time.perf_counter() - t0) * 1e6)
        lines.append(f"k={k} assign {med(t_new) / 1e3:.2f} ms | host GEMM-argmin {med(t_old) / 1e3:.2f} ms: ratio {med(t_old) / med(t_new):.1f}x, "
                     f"{verdict(t_new, t_old)}")
        flush()
        us = timed(aspace, lambda: aspace.assign(C))
        kp, dp, npad = (k + 63) // 64 * 64, (d + 31) // 32 * 32, (n + 127) // 128 * 128
        lines.append(f"k={k} assign launches (centroid norms + fused GEMM-argmin) by HIP events {us[0] / 1e3:.2f} ms: "
                     f"{2.0 * npad * kp * dp / (us[0] * 1e-6) / PEAK:.2f} of the fp64 MFMA peak (subset_score_batch_kernel: 0.58-0.63)")
        flush()
        # Lloyd
        cent, lab, info = aspace.kmeans(k, seed=0, max_iters=LLOYD_ITERS, with_info=True)
        hc, hl = host_kmeans(X, nx, C, LLOYD_ITERS)
        same = bool(np.array_equal(lab, hl))
        lines.append(f"k={k} kmeans: {info['iterations']} iterations, changed {info['changed']}, empty {info['empty']}, inertia {info['inertia']:.6f}; "
                     f"labels {'equal the host loop' if same else 'differ from the host loop at %d items (near-ties)' % int((lab != hl).sum())}, centroids "
                     f"{'equal it in bits' if np.array_equal(cent, hc) else 'differ by at most %.3g' % float(np.abs(cent - hc).max())}")
        flush()
        t_new, t_old = [], []
        for _ in range(rounds):
            t0 = time.perf_counter()
            aspace.kmeans(k, seed=0, max_iters=LLOYD_ITERS)
            t_new.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            host_kmeans(X, nx, C, LLOYD_ITERS)
            t_old.append((time.perf_counter() - t0) * 1e6)
        lines.append(f"k={k} kmeans {med(t_new) / 1e3:.2f} ms | host loop with kmeans_ref.update {med(t_old) / 1e3:.2f} ms: ratio "
                     f"{med(t_old) / med(t_new):.1f}x, {verdict(t_new, t_old)}")
        flush()
        us = timed(aspace, lambda: aspace.kmeans(k, seed=0, max_iters=LLOYD_ITERS))
        its = max(us[3], 1.0)
        moved = n * d * 4 + 2 * (n / 256 + k) * d * 8 + 2 * k * d * 8 + n * 4
        lines.append(f"k={k} per iteration by HIP events: assign {us[0] / its / 1e3:.2f} ms, ordering (clear, histogram, scan, scatter) "
                     f"{us[1] / its:.1f} us, update (segment sums, final) {us[2] / its:.1f} us = {moved / 1e6:.0f} MB at "
                     f"{moved / (us[2] / its * 1e-6) / HBM:.2f} of 8 TB/s")
        flush()
    # the route through the score kernel: one tile of centroids over all ids, k x N scores to the host
    ids_all = np.arange(n)
    served = []   # (an item without a neighbour inside eps has lambda_q = 0 and is not scored)
    for i in range(n):
        if aspace.query_lambda(np.ascontiguousarray(X[i]), gl) != 0.0:
            served.append(i)
            if len(served) == 64:
                break
    Q = np.ascontiguousarray(X[served])
    aspace.score_items_batch(Q, gl, 0.62, ids_all)
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        aspace.score_items_batch(Q, gl, 0.62, ids_all)
        ts.append((time.perf_counter() - t0) * 1e6)
    lines.append(f"score_items_batch over all ids, 64 vectors: {med(ts) / 1e3:.2f} ms = {med(ts) / 64 / 1e3:.2f} ms per centroid (blended cosine scores, "
                 f"not distances; the 64 x N matrix crosses to the host)")
    lines.append(f"kmeans_counters {aspace.kmeans_counters()}")
    flush()


if __name__ == "__main__":
    main()
