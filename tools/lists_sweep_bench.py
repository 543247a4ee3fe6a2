"""Tau sweeps over per-query candidate lists at the headline size: `search_batch_lists_taus` / `score_lists_batch_taus` under T taus
against what a caller had before -- the loop of T back-to-back `search_batch_lists` / `score_lists_batch` calls over the same lists.
python tools/lists_sweep_bench.py [N] [D] [OUT]  (defaults 1M x 768, profiles/r12_lists_sweep.txt).

Index, queries and lists are those of tools/lists_bench.py (clustered Gaussians by the torch RNG, seed 42; L2 / Gaussian, k = 25,
topk = 15; bench.make_queries, seed 43; lists drawn with seed 45): (B, C) in {(1024, 100), (1024, 1000), (128, 10000)} and 1024
ragged lists with lengths log-uniform in [10, 10000].  T = 3 (taus 1, .8, .62, the reference harnesses' three) and T = 6.  Per cell
(case, T, form) the sweep's results are checked against the loop's first (scores 1e-12 relative, `==` for taus[0]; lists through
`same_as_single`), both are warmed up, then the sweep and the loop ALTERNATE in one process, REPS times each; medians.  Recorded
per cell: the two call times and their ratio, the score kernel's device time by HIP events summed over the launches of a call
(sweep: one gather per group of taus; loop: T gathers), and the serial host share (id checks, wait for the deduplication, work
tables: slot [5] of as_lists_sweep_counters, `lists_counters()['host_ns']` for the loop).  The objects alive after the set-up are
frozen out of Python's garbage collector (gc.freeze): the search forms return thousands of tuples per call, and every few calls
that triggered a full collection over torch's and numpy's objects -- some 40 ms that fell on the sweep or on the loop by turns."""
import gc
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from lists_bench import draw_list  # noqa: E402
from subset_bench import same_as_single  # noqa: E402
from tau_sweep_bench import gpu_clustered  # noqa: E402

REPS = 5
TAU_SETS = ([1.0, 0.8, 0.62], [1.0, 0.8, 0.62, 0.4, 0.2, 0.0])


def sweep_host_ns(aspace):
    out = np.zeros(6, dtype=np.int64)
    assert asp._L.as_lists_sweep_counters(aspace._h, out.ctypes.data, 6) == 0
    return int(out[5])


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    out = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "r12_lists_sweep.txt")
    X = gpu_clustered(n, d, 42)
    gp = {"eps": bench.calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = np.ascontiguousarray(np.stack([np.ascontiguousarray(q) for q in bench.make_queries(X, 1024, 43)]))
    del X
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    rng = np.random.default_rng(45)
    lines = [f"search_batch_lists_taus / score_lists_batch_taus against the loop of T single-tau calls: N={n} D={d} k=25 topk=15 l2/gaussian "
             f"eps={gp['eps']:.5f}; sweep and loop alternate in one process after a warm-up of both, medians of {REPS}; kernel = the score "
             f"kernel by HIP events summed over the launches of a call (loop: over its T calls); host = serial host time of a call (id "
             f"checks, wait for the deduplication, work tables)"]
    print(lines[0], flush=True)
    cases = [("B=1024 C=100", 1024, lambda: 100), ("B=1024 C=1000", 1024, lambda: 1000), ("B=128 C=10000", 128, lambda: 10000),
             ("B=1024 ragged 10..10000", 1024, lambda: int(round(10.0 ** rng.uniform(1.0, 4.0))))]
    missed = []
    for name, b, length in cases:
        Qb = np.ascontiguousarray(Q[:b])
        lists = [draw_list(rng, n, length()) for _ in range(b)]
        total = int(sum(len(l) for l in lists))
        arg = np.stack(lists) if len({len(l) for l in lists}) == 1 else lists
        for taus in TAU_SETS:
            T = len(taus)
            forms = (("search", lambda: aspace.search_batch_lists_taus(Qb, gl, taus, arg),
                      lambda: [aspace.search_batch_lists(Qb, gl, tau, arg) for tau in taus]),
                     ("score", lambda: aspace.score_lists_batch_taus(Qb, gl, taus, arg),
                      lambda: [aspace.score_lists_batch(Qb, gl, tau, arg) for tau in taus]))
            for form, sweep, loop in forms:
                got, want = sweep(), loop()   # warm-up of both (the buffers are made here), and the check
                for i in range(b):
                    for j in range(T):
                        if form == "search":
                            same_as_single(got[i][j], want[j][i])
                        else:
                            np.testing.assert_allclose(got[i][j], want[j][i], rtol=1e-12, atol=0.0)
                    if form == "search":
                        assert got[i][0] == want[0][i]
                    else:
                        assert np.array_equal(got[i][0], want[0][i])
                del got, want
                assert asp._L.as_set_tuning(b"lists_timing", 1) == 0
                try:
                    ts, tl, ks, kl, hs, hl = [], [], [], [], [], []
                    for _ in range(REPS):
                        h0 = sweep_host_ns(aspace)
                        t0 = time.perf_counter()
                        sweep()
                        ts.append((time.perf_counter() - t0) * 1e6)
                        ks.append(asp._L.as_lists_kernel_us(aspace._h))
                        hs.append((sweep_host_ns(aspace) - h0) / 1e3)
                        h0 = aspace.lists_counters()["host_ns"]
                        k, t_all = 0.0, 0.0
                        for tau in taus:   # the loop, call by call: the kernel time of each call is read after it
                            t0 = time.perf_counter()
                            if form == "search":
                                aspace.search_batch_lists(Qb, gl, tau, arg)
                            else:
                                aspace.score_lists_batch(Qb, gl, tau, arg)
                            t_all += (time.perf_counter() - t0) * 1e6
                            k += asp._L.as_lists_kernel_us(aspace._h)
                        tl.append(t_all)
                        kl.append(k)
                        hl.append((aspace.lists_counters()["host_ns"] - h0) / 1e3)
                finally:
                    assert asp._L.as_set_tuning(b"lists_timing", 0) == 0
                print(f"  {name} T={T} {form}: sweep calls {[round(v) for v in ts]} us, loops {[round(v) for v in tl]} us", flush=True)
                ts, tl, ks, kl, hs, hl = (float(np.median(v)) for v in (ts, tl, ks, kl, hs, hl))
                verdict = "below the loop" if ts < tl else "NOT below the loop"
                if ts >= tl:
                    missed.append(f"{name} T={T} {form}")
                lines.append(f"{name} T={T} {form} form: sum(m_i)={total} | sweep {ts:.0f} us = {ts / b:.1f} us/query | loop of {T} calls {tl:.0f} us = "
                             f"{tl / b:.1f} us/query | loop / sweep = {tl / ts:.2f} ({verdict}) | score kernel: sweep {ks:.1f} us, loop {kl:.1f} us | "
                             f"host: sweep {hs:.0f} us = {hs / ts:.3f} of the call, loop {hl:.0f} us = {hl / tl:.3f}")
                print(lines[-1], flush=True)
    lines.append("cells whose sweep median is not below the loop's: " + (", ".join(missed) if missed else "none"))
    lines.append(f"lists_sweep_counters {aspace.lists_sweep_counters()}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-2])
    print(lines[-1])


if __name__ == "__main__":
    main()
