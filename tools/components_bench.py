"""Connected components of the item graph at the headline size: `ArrowSpace.components` and
`components_sweep` against the route there was before -- scipy.sparse.csgraph.connected_components over `to_csr()`'s matrix, prepared
(and, for a threshold, filtered by `to_csr_dist()`) outside the timing -- the two routes alternating in one process.
python tools/components_bench.py [N] [D] [ROUNDS] [OUT]  (defaults 1M x 768, 5 rounds, profiles/r24_components.txt).

Data and index: tools/diffuse_bench.py's (clustered Gaussians, k = 25, topk = 100).  Every answer is checked first against the
baseline's partition, its labels canonicalised to smallest ids.  Cells: no threshold; one threshold at the median stored distance;
a sweep of 8 thresholds at the octiles of the stored distances, timed against 8 single calls and against 8 baseline calls.
Criterion, the project's own: the new call's median is below the baseline's by more than the baseline's own spread.  Then, by HIP
events ("diffuse_timing", a separate pass): hook, compress and statistics time per round, the rounds taken, and the hook's bytes (4
per entry, 12 when filtered, plus indptr) against the 8 TB/s peak."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import scipy.sparse as sps  # noqa: E402
import torch  # noqa: E402
from scipy.sparse.csgraph import connected_components  # noqa: E402

import components_ref as cr  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, med  # noqa: E402

L = asp._L
PEAK = 8e12


def verdict(new, old):
    spread = max(old) - min(old)
    ok = med(new) < med(old) - spread
    return (f"baseline spread {spread / 1e3:.2f} ms: " +
            ("the new call is below the baseline by more than it" if ok else "the new call is NOT below the baseline by more than its spread"))


def numbers(labels):
    """count, largest, largest_label, isolated of canonical labels."""
    sizes = np.bincount(labels, minlength=labels.shape[0])
    big = int(sizes.max())
    return {"count": int((sizes > 0).sum()), "largest": big, "largest_label": int(np.flatnonzero(sizes == big)[0]), "isolated": int((sizes == 1).sum())}


class Host:
    """The baseline: scipy over the stored entries; the matrices are made outside the timing."""

    def __init__(self, ip, ci, dist):
        self.n, self.ip, self.ci, self.dist = ip.shape[0] - 1, ip, ci, dist
        self.rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(ip))
        self.mats = {}

    def matrix(self, t):
        if t not in self.mats:
            keep = slice(None) if t is None else self.dist <= t
            r, c = self.rows[keep], self.ci[keep]
            self.mats[t] = (sps.csr_matrix((np.ones(r.shape[0], dtype=np.int8), (r, c)), shape=(self.n, self.n)), int(r.shape[0]))
        return self.mats[t]

    def run(self, t):
        """-> (labels as scipy numbers them, microseconds)"""
        A = self.matrix(t)[0]
        t0 = time.perf_counter()
        lab = connected_components(A, directed=True, connection="weak")[1]
        return lab, (time.perf_counter() - t0) * 1e6


def checked(aspace, gl, host, t):
    """One call checked against the baseline's partition -> its info."""
    labels, info = aspace.components(gl, t, with_info=True)
    want = cr.canonical(host.run(t)[0])
    assert np.array_equal(labels, want), ("labels differ from the baseline's partition", t)
    assert {k: info[k] for k in ("count", "largest", "largest_label", "isolated")} == numbers(want), (info, numbers(want))
    assert info["edges_kept"] == host.matrix(t)[1]
    return info


def single_cell(aspace, gl, host, t, name, rounds, lines):
    info = checked(aspace, gl, host, t)   # the answer, and the warm-up
    t_new, t_old = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        aspace.components(gl, t)
        t_new.append((time.perf_counter() - t0) * 1e6)
        t_old.append(host.run(t)[1])
    lines.append(f"{name}: components {med(t_new) / 1e3:.2f} ms ({info['rounds']} rounds; {info['count']} components, the largest {info['largest']} items "
                 f"(label {info['largest_label']}), {info['isolated']} isolated, {info['edges_kept']} entries kept) | scipy connected_components "
                 f"{med(t_old) / 1e3:.2f} ms: ratio {med(t_old) / med(t_new):.1f}x, {verdict(t_new, t_old)}")
    print(lines[-1], flush=True)
    return info


def sweep_cell(aspace, gl, host, ts, rounds, lines):
    singles = [checked(aspace, gl, host, t) for t in ts]
    got = aspace.components_sweep(gl, ts)
    for k in ("count", "largest", "largest_label", "isolated", "edges_kept"):
        assert got[k].tolist() == [s[k] for s in singles], k
    t_sweep, t_single, t_old = [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        aspace.components_sweep(gl, ts)
        t_sweep.append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        for t in ts:
            aspace.components(gl, t)
        t_single.append((time.perf_counter() - t0) * 1e6)
        t_old.append(sum(host.run(t)[1] for t in ts))
    lines.append(f"sweep of {len(ts)} thresholds at the octiles of the stored distances: components_sweep {med(t_sweep) / 1e3:.2f} ms "
                 f"({int(got['rounds'].sum())} rounds in all; components per threshold {got['count'].tolist()}) | {len(ts)} single calls "
                 f"{med(t_single) / 1e3:.2f} ms ({sum(s['rounds'] for s in singles)} rounds): ratio {med(t_single) / med(t_sweep):.2f}x, "
                 f"{verdict(t_sweep, t_single).replace('baseline', 'single calls')} | {len(ts)} scipy calls {med(t_old) / 1e3:.2f} ms: ratio "
                 f"{med(t_old) / med(t_sweep):.1f}x, {verdict(t_sweep, t_old)}")
    print(lines[-1], flush=True)


def events_cell(aspace, gl, t, name, n, nnz, lines):
    assert L.as_set_tuning(b"diffuse_timing", 1) == 0
    try:
        aspace.components(gl, t)   # (warm-up)
        aspace.components(gl, t)
        us = [L.as_components_kernel_us(aspace._h, p) for p in range(4)]
    finally:
        assert L.as_set_tuning(b"diffuse_timing", 0) == 0
    r = int(us[3])
    per_round = (4 if t is None else 12) * nnz + 8 * (n + 1)
    rate = per_round * r / (us[0] * 1e-6)
    lines.append(f"{name} by HIP events (every round timed, so the call is slower than untimed): {r} rounds; hook {us[0] / r:.1f} us per round, "
                 f"compress {us[1] / r:.1f} us per round, statistics {us[2]:.1f} us per call; the hook streams {per_round / 1e6:.1f} MB per round: "
                 f"{rate / 1e12:.2f} TB/s, {100 * rate / PEAK:.0f}% of the 8 TB/s peak (rounds after the first gather from a parent that no longer "
                 f"changes); a diffusion step at C = 1 is 357 us")
    print(lines[-1], flush=True)


def main():
    argv = sys.argv[1:]
    n_items = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    rounds = int(argv[2]) if len(argv) > 2 else 5
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r24_components.txt")
    X = gpu_clustered(n_items, d, 42)
    eps = calibrate_eps(X, 25)
    gp = {"eps": eps, "k": 25, "topk": 100, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n_items, d, d)
    torch.cuda.synchronize()
    ip, ci, dist = gl.to_csr_dist()
    host = Host(ip, ci, dist)
    deg = np.diff(ip)
    lines = [f"components vs scipy.sparse.csgraph.connected_components on the host over the stored entries: N={n_items} D={d} k=25 topk=100 l2/gaussian "
             f"eps={eps:.5f}; {len(ci)} stored entries, longest row {int(deg.max())}, {int((deg == 0).sum())} rows without an entry; stored distances "
             f"{dist.min():.5f} .. {dist.max():.5f}; {rounds} rounds alternating, medians"]
    print(lines[0], flush=True)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

    info = single_cell(aspace, gl, host, None, "no threshold", rounds, lines)
    lines.append(f"the graph of r21-r23 has {info['count']} components ({info['isolated']} of them single items): the count eigsh's m <= 48 could not give")
    flush()
    median = float(np.median(dist))
    single_cell(aspace, gl, host, median, f"max_dist = the median stored distance {median:.5f}", rounds, lines)
    flush()
    octiles = [float(v) for v in np.quantile(dist, np.arange(1, 9) / 8.0)]
    sweep_cell(aspace, gl, host, octiles, rounds, lines)
    flush()
    host.mats.clear()
    events_cell(aspace, gl, None, "no threshold", n_items, len(ci), lines)
    events_cell(aspace, gl, median, "max_dist = the median", n_items, len(ci), lines)
    lines.append(f"components_counters {aspace.components_counters()}")
    flush()


if __name__ == "__main__":
    main()
