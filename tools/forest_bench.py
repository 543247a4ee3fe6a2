"""Minimum spanning forest of the item graph at the headline size: `ArrowSpace.spanning_forest`
against the route there was before -- scipy.sparse.csgraph.minimum_spanning_tree over the min-symmetrised matrix of
`to_csr_dist()`, prepared outside the timing -- the two routes alternating in one process.
python tools/forest_bench.py [N] [D] [ROUNDS] [OUT]  (defaults 1M x 768, 5 rounds, profiles/r25_forest.txt).

Data and index: tools/diffuse_bench.py's (clustered Gaussians, k = 25, topk = 100).  The new call's answer is checked first, edge
by edge and in bits, against tests/forest_ref.py's Kruskal (not against scipy, which drops zero weights and breaks ties its own
way; only the two edge counts and total weights are printed side by side).  Criterion, the project's own: the new call's median
is below the baseline's by more than the baseline's own spread.  Then, by HIP events ("diffuse_timing", separate passes): the four
launches of every round, init + weights, emit, the host's sort, and the row-minimum kernel at 8 / 16 / 32 lanes per row."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import scipy.sparse as sps  # noqa: E402
import torch  # noqa: E402
from scipy.sparse.csgraph import minimum_spanning_tree  # noqa: E402

import forest_ref as fr  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from components_bench import verdict  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, med  # noqa: E402

L = asp._L
NAMES = ("rowmin", "pick", "link", "compress")


def timed(aspace, gl, lanes=0):
    """One call under "diffuse_timing" (after a warm-up) -> as_forest_kernel_us's parts."""
    assert L.as_set_tuning(b"forest_row_lanes", lanes) == 0 and L.as_set_tuning(b"diffuse_timing", 1) == 0
    try:
        aspace.spanning_forest(gl)
        aspace.spanning_forest(gl)
        return [L.as_forest_kernel_us(aspace._h, p) for p in range(8 + 4 * 32)]
    finally:
        assert L.as_set_tuning(b"diffuse_timing", 0) == 0 and L.as_set_tuning(b"forest_row_lanes", 0) == 0


def main():
    argv = sys.argv[1:]
    n_items = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    rounds = int(argv[2]) if len(argv) > 2 else 5
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r25_forest.txt")
    X = gpu_clustered(n_items, d, 42)
    eps = calibrate_eps(X, 25)
    gp = {"eps": eps, "k": 25, "topk": 100, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n_items, d, d)
    torch.cuda.synchronize()
    ip, ci, dist = gl.to_csr_dist()
    lines = [f"spanning_forest vs scipy.sparse.csgraph.minimum_spanning_tree on the host over the min-symmetrised stored entries: N={n_items} D={d} "
             f"k=25 topk=100 l2/gaussian eps={eps:.5f}; {len(ci)} stored entries; {rounds} rounds alternating, medians"]
    print(lines[0], flush=True)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

    # the answer first: Kruskal under the total order on the stored CSR
    (u, v, w), info = aspace.spanning_forest(gl, with_info=True)
    t0 = time.perf_counter()
    want = fr.kruskal(n_items, ip, ci, dist)
    t_ref = time.perf_counter() - t0
    assert np.array_equal(u, want[0]) and np.array_equal(v, want[1]) and np.array_equal(w.view(np.int64), want[2].view(np.int64))
    count = aspace.components(gl, with_info=True)[1]["count"]
    assert info["edges"] == n_items - count
    lines.append(f"the answer equals the numpy Kruskal's in u, v, the bits of dist and order ({t_ref:.1f} s on the host): {info['edges']} edges, "
                 f"{info['components']} components (components() counts {count}), {info['rounds']} rounds; weights {w.min():.5f} .. {w.max():.5f}")
    print(lines[-1], flush=True)
    flush()
    # the baseline's matrix, outside the timing: every undirected edge once, in both directions, with the smaller dist
    eu, ev, ew = fr.edges(n_items, ip, ci, dist)
    A = sps.csr_matrix((np.concatenate([ew, ew]), (np.concatenate([eu, ev]), np.concatenate([ev, eu]))), shape=(n_items, n_items))
    t_new, t_raw, t_old = [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        aspace.spanning_forest(gl)
        t_new.append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        aspace.spanning_forest(gl, sort=False)
        t_raw.append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        T = minimum_spanning_tree(A)
        t_old.append((time.perf_counter() - t0) * 1e6)
    lines.append(f"spanning_forest {med(t_new) / 1e3:.2f} ms sorted, {med(t_raw) / 1e3:.2f} ms in slot order | scipy minimum_spanning_tree "
                 f"{med(t_old) / 1e3:.2f} ms ({T.nnz} edges of total weight {T.sum():.6f}; the new call's {len(w)} edges sum to {w.sum():.6f}): ratio "
                 f"{med(t_old) / med(t_new):.1f}x, {verdict(t_new, t_old)}")
    print(lines[-1], flush=True)
    flush()
    us = timed(aspace, gl)
    r = int(us[7])
    lines.append(f"by HIP events (every launch timed and a wait after the weights, so the call is slower than untimed), {r} rounds: init + weights "
                 f"{us[4]:.1f} us, " + ", ".join(f"{nm} {us[k]:.1f} us" for k, nm in enumerate(NAMES)) + f" over the rounds, emit {us[5]:.1f} us; the host's "
                 f"sort {us[6]:.1f} us")
    for i in range(min(r, 32)):
        lines.append(f"  round {i + 1}: " + ", ".join(f"{nm} {us[8 + 4 * i + k]:.1f} us" for k, nm in enumerate(NAMES)))
    by_lanes = {lanes: [timed(aspace, gl, lanes)[0] for _ in range(3)] for lanes in (8, 16, 32)}
    best = min(by_lanes, key=lambda k: med(by_lanes[k]))
    lines.append("row-minimum kernel over the rounds by lanes per row (medians of 3): " + ", ".join(f"W = {k}: {med(t):.1f} us" for k, t in by_lanes.items())
                 + f"; the fastest is W = {best}")
    lines.append(f"spanning_forest_counters {aspace.spanning_forest_counters()}")
    print("\n".join(lines[-r - 3:]), flush=True)
    flush()


if __name__ == "__main__":
    main()
