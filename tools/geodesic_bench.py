"""Shortest paths over the item graph at the headline size: `ArrowSpace.shortest_paths` and
`search_geodesic` against the route there was before -- scipy.sparse.csgraph.dijkstra over the min-symmetrised matrix of
`to_csr_dist()`, prepared outside the timing -- the routes alternating in one process.
python tools/geodesic_bench.py [N] [D] [ROUNDS] [OUT]  (defaults 1M x 768, 5 rounds, profiles/r26_geodesic.txt).

Data and index: tools/diffuse_bench.py's (clustered Gaussians, k = 25, topk = 100).  Every answer is checked first, in bits: the
one-source block against scipy's (the same float64 add; the least fixed point is unique) and, under the cutoff, against
tests/geodesic_ref.py's heap Dijkstra; the 64-source block against scipy's.  Criterion, the project's own: the new call's median is
below the baseline's by more than the baseline's own spread.  The 64-source baseline takes minutes: it runs min(ROUNDS, 2) times.
Then, by HIP events ("diffuse_timing", separate passes): the parts of as_geodesic_kernel_us with the bytes the pull rounds moved, and the one-source call under the row
lanes, the LDS rows and the bucket widths."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import scipy.sparse as sps  # noqa: E402
import torch  # noqa: E402
from scipy.sparse.csgraph import dijkstra  # noqa: E402

import forest_ref as fr  # noqa: E402
import geodesic_ref as gr  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from components_bench import verdict  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, med  # noqa: E402

L = asp._L
PARTS = ("weights", "LDS rounds", "grid-wide relax", "filter", "pull rounds", "emit (host)")


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e6


def timed(aspace, gl, sources, lanes=0, lds_rows=-1, delta=0.0, cutoff=None):
    """One call under "diffuse_timing" (after a warm-up) -> (as_geodesic_kernel_us's parts, the call's wall microseconds untimed)."""
    assert L.as_set_tuning(b"geodesic_row_lanes", lanes) == 0 and L.as_set_tuning(b"geodesic_lds_rows", lds_rows) == 0
    L.as_set_geodesic_delta(delta)
    try:
        aspace.score_geodesic(gl, sources, [0], cutoff)
        wall = med([clock(lambda: aspace.score_geodesic(gl, sources, [0], cutoff))[1] for _ in range(3)])
        assert L.as_set_tuning(b"diffuse_timing", 1) == 0
        aspace.score_geodesic(gl, sources, [0], cutoff)
        return [L.as_geodesic_kernel_us(aspace._h, p) for p in range(12)], wall
    finally:
        assert L.as_set_tuning(b"diffuse_timing", 0) == 0 and L.as_set_tuning(b"geodesic_row_lanes", 0) == 0
        assert L.as_set_tuning(b"geodesic_lds_rows", -1) == 0
        L.as_set_geodesic_delta(0.0)


def spread(aspace, gl, sources, **tuning):
    """The untimed wall of the score form under a tuning, 9 calls -> "median (min .. max) ms"."""
    t = [timed(aspace, gl, sources, **tuning)[1] for _ in range(3)]   # (each a median of 3)
    return f"{med(t) / 1e3:.3f} ({min(t) / 1e3:.3f} .. {max(t) / 1e3:.3f}) ms"


def main():
    argv = sys.argv[1:]
    n_items = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    rounds = int(argv[2]) if len(argv) > 2 else 5
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r26_geodesic.txt")
    X = gpu_clustered(n_items, d, 42)
    eps = calibrate_eps(X, 25)
    gp = {"eps": eps, "k": 25, "topk": 100, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n_items, d, d)
    torch.cuda.synchronize()
    ip, ci, dist = gl.to_csr_dist()
    lines = [f"shortest_paths / search_geodesic vs scipy.sparse.csgraph.dijkstra on the host over the min-symmetrised stored entries: N={n_items} "
             f"D={d} k=25 topk=100 l2/gaussian eps={eps:.5f}; {len(ci)} stored entries; {rounds} rounds alternating, medians; the defaults: 16 lanes per frontier row, 2048 LDS rows, one bucket, 64 columns"]

    def say(text):
        lines.append(text)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

    print(lines[0], flush=True)
    # the baseline's matrix, outside the timing: every undirected edge once, in both directions, with the smaller dist
    eu, ev, ew = fr.edges(n_items, ip, ci, dist)
    A = sps.csr_matrix((np.concatenate([ew, ew]), (np.concatenate([eu, ev]), np.concatenate([ev, eu]))), shape=(n_items, n_items))
    labels = aspace.components(gl)
    big = int(np.bincount(labels).argmax())
    rng = np.random.default_rng(3)
    src1 = [int(rng.choice(np.flatnonzero(labels == big)))]
    src64 = [int(i) for i in rng.choice(n_items, 64, replace=False)]
    cutoff = float(np.median(dist))
    # the answers first
    d1, info1 = aspace.shortest_paths(gl, src1, with_info=True)
    want1 = dijkstra(A, directed=False, indices=src1)
    assert same(d1, want1)
    ball = aspace.shortest_paths(gl, src1, cutoff)
    w_entries = gr.weights(n_items, ip, ci, dist)
    assert same(ball[0], gr.dijkstra(n_items, ip, ci, w_entries, src1, [0.0], cutoff)) and same(ball, np.where(want1 <= cutoff, want1, np.inf))
    say(f"one source (item {src1[0]} of the largest component, {int((labels == big).sum())} items): the block equals scipy's in bits, and under "
        f"cutoff {cutoff:.5f} (the median stored dist) the heap Dijkstra's of tests/geodesic_ref.py: {int(info1['reached'][0])} reached, "
        f"{int(np.isfinite(ball).sum())} inside the cutoff, rounds {info1['rounds']}, {info1['relaxations']} relaxations, max d {d1[np.isfinite(d1)].max():.5f}")
    t_new64, t_old64 = [], []
    for r in range(min(rounds, 2)):
        (d64, info64), t = clock(lambda: aspace.shortest_paths(gl, src64, with_info=True))
        t_new64.append(t)
        want64, t = clock(lambda: dijkstra(A, directed=False, indices=src64))
        t_old64.append(t)
        assert same(d64, want64)
    t_new64 += [clock(lambda: aspace.shortest_paths(gl, src64))[1] for _ in range(rounds - len(t_new64))]
    say(f"64 sources: the block equals scipy's in bits; reached per column {int(info64['reached'].min())} .. {int(info64['reached'].max())}, rounds "
        f"{info64['rounds']}")
    q = X[src1[0]].double().cpu().numpy()
    t_new1, t_old1, t_s, t_sc = [], [], [], []
    for _ in range(rounds):
        t_new1.append(clock(lambda: aspace.shortest_paths(gl, src1))[1])
        t_old1.append(clock(lambda: dijkstra(A, directed=False, indices=src1))[1])
        t_s.append(clock(lambda: aspace.search_geodesic(q, gl, 0.62))[1])
        t_sc.append(clock(lambda: aspace.search_geodesic(q, gl, 0.62, cutoff=cutoff))[1])
    t_search = med([clock(lambda: aspace.search(q, gl, 0.62))[1] for _ in range(rounds)])
    say(f"shortest_paths, 1 source {med(t_new1) / 1e3:.2f} ms | scipy dijkstra {med(t_old1) / 1e3:.2f} ms: ratio {med(t_old1) / med(t_new1):.1f}x, "
        f"{verdict(t_new1, t_old1)}")
    say(f"shortest_paths, 64 sources {med(t_new64) / 1e3:.2f} ms (of {len(t_new64)}) | scipy dijkstra {med(t_old64) / 1e3:.2f} ms (of {len(t_old64)} runs: "
        f"{', '.join(f'{t / 1e3:.0f}' for t in t_old64)} ms): ratio {med(t_old64) / med(t_new64):.1f}x"
        + (f", {verdict(t_new64, t_old64)}" if len(t_old64) > 1 else ""))
    say(f"search_geodesic {med(t_s) / 1e3:.2f} ms, with cutoff {cutoff:.5f} {med(t_sc) / 1e3:.2f} ms (the ordinary search alone {t_search / 1e3:.2f} ms) | "
        f"scipy dijkstra alone {med(t_old1) / 1e3:.2f} ms: {verdict(t_s, t_old1)}")
    nnz = len(ci)
    for what, src, cut in (("1 source", src1, None), ("1 source under the cutoff", src1, cutoff), ("64 sources", src64, None)):
        us, wall = timed(aspace, gl, src, cutoff=cut)
        text = ", ".join(f"{nm} {us[k]:.1f} us" for k, nm in enumerate(PARTS))
        if us[8] > 0:   # every row scans its columns and their stamps (8 B per entry); a row that relaxes reads the columns again and the
            # weight images (12 B per entry) and gathers a segment of 8 C bytes per entry (C = 64: the one chunk of the 64 sources)
            csr, seg = us[8] * 8 + us[11] * 12, us[11] * 8 * 64
            text += (f"; the pull rounds scanned {us[8]:.0f} entries and relaxed rows of {us[11]:.0f}: {csr / 1e9:.3f} GB of CSR and {seg / 1e9:.3f} GB of "
                     f"gathered segments, {(csr + seg) / (us[4] * 1e-6) / 1e12:.2f} TB/s of 8 TB/s")
        say(f"by HIP events, {what} (score form, {wall / 1e3:.2f} ms untimed): {text}; {int(us[7])} rounds, {int(us[9])} one-block and {int(us[10])} "
            f"grid-wide launches, weights launches {int(us[6])}")
    L.as_set_tuning(b"diffuse_timing", 1)
    aspace.spanning_forest(gl)   # (another graph's images would be replaced; the forest's own launch, for the weights' time)
    say(f"the weights launch (as_forest_kernel_us part 4, init + weights): {L.as_forest_kernel_us(aspace._h, 4):.1f} us, "
        f"{nnz * 36 / (L.as_forest_kernel_us(aspace._h, 4) * 1e-6) / 1e12:.2f} TB/s over 36 B per entry")
    L.as_set_tuning(b"diffuse_timing", 0)
    pos = np.sort(w_entries[w_entries > 0.0])
    say("one source by the tunings (untimed wall, medians of 3; W: the median, least and most of three such medians): " + "; ".join(
        [f"W = {k}: {spread(aspace, gl, src1, lanes=k)}" for k in (8, 16, 32)]
        + [f"R = {k}: {timed(aspace, gl, src1, lds_rows=k)[1] / 1e3:.2f} ms" for k in (0, 512, 2048, 4096)]
        + [f"delta = {k:.4g}: {timed(aspace, gl, src1, delta=k)[1] / 1e3:.2f} ms" for k in (0.0, float(pos[len(pos) // 2]), float(4 * pos[len(pos) // 2]))]))
    L.as_set_tuning(b"diffuse_cols", 16)
    t16 = med([clock(lambda: aspace.score_geodesic(gl, src64, [0]))[1] for _ in range(3)])
    L.as_set_tuning(b"diffuse_cols", 0)
    t64 = med([clock(lambda: aspace.score_geodesic(gl, src64, [0]))[1] for _ in range(3)])
    say(f"64 sources in chunks of 16 columns {t16 / 1e3:.2f} ms, in one chunk of 64 {t64 / 1e3:.2f} ms (score form, medians of 3)")
    say(f"geodesic_counters {aspace.geodesic_counters()}")


if __name__ == "__main__":
    main()
