"""Fused multi-query search at the headline size: `search_fused` / `score_fused` against the only route there was before them --
`score_items_batch` of the J vectors over the ids (a J x M matrix of fp64 scores to host memory), `fused_ref.fuse` and
`fused_ref.top` in numpy -- per need (a group of J vectors), alternating in one process, and the accumulate kernel's own
duration by HIP events (as_set_tuning("fused_timing")).
python tools/fused_bench.py [N] [D] [NEEDS] [ROUNDS] [OUT]  (defaults 1M x 768, 8 needs, 5 rounds, profiles/r15_fused.txt).

Data: clustered Gaussians around 1 024 centres, rows normalised, fp32 (torch RNG, seed 42), L2 distance / Gaussian weights,
k = 25, topk = 15, tau = 0.62, eps such that a row has about 2 k items inside it; a need: J perturbed items (seed 43), weights
1/J, mode sum.  Cells: J = 2, 8, 32 over a prepared subset of M = 1 000 and 100 000 uniformly random items and all N
(subset=None).  Every need's answer is checked against the baseline's (indices and score bits, both modes) before it is timed.
Reports the medians of both forms and of their baselines over needs x rounds, and the accumulate kernel's median microseconds
and GB/s over the J x M x 8 bytes it reads (a separate pass with the events on)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fused_ref  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, make_queries, med  # noqa: E402

TAU = 0.62
JS = (2, 8, 32)


def same_hits(got, ids, F, k):
    wi, ws = fused_ref.top(ids, F, k)
    assert [i for i, _ in got] == wi.tolist(), (len(got), len(wi))
    assert np.array([v for _, v in got]).tobytes() == ws.tobytes()


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    needs = int(argv[2]) if len(argv) > 2 else 8
    rounds = int(argv[3]) if len(argv) > 3 else 5
    out = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "r15_fused.txt")
    X = gpu_clustered(n, d, 42)
    gp = {"eps": calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = make_queries(X, needs * max(JS), 43)
    del X
    torch.cuda.synchronize()
    L = asp._L
    topk = gp["topk"]
    rng = np.random.default_rng(44)
    lines = [f"search_fused / score_fused vs score_items_batch + numpy fuse (+ lexsort): N={n} D={d} k=25 topk={topk} l2/gaussian "
             f"eps={gp['eps']:.5f} tau={TAU}, weights 1/J, mode sum, {needs} needs x {rounds} rounds alternating; kernel = "
             f"fused_accumulate_kernel by HIP events (separate pass), GB/s over the J*M*8 bytes of scores it reads"]
    worse = []
    for m in sorted({min(1_000, n), min(100_000, n), n}):
        ids = np.arange(n) if m == n else np.sort(rng.choice(n, m, replace=False))
        sub = None if m == n else aspace.subset(ids)
        for J in JS:
            groups = [np.ascontiguousarray(Q[g * J:(g + 1) * J]) for g in range(needs)]
            w = np.full(J, 1.0 / J)
            for G in groups:   # the answers, and the warm-up
                S = aspace.score_items_batch(G, gl, TAU, ids)
                for mode in ("sum", "max"):
                    F = fused_ref.fuse(S, w, mode)
                    assert aspace.score_fused(G, gl, TAU, ids, mode=mode).tobytes() == F.tobytes()
                    same_hits(aspace.search_fused(G, gl, TAU, mode=mode, subset=sub), ids, F, topk)
                del S
            t_search, t_score, b_search, b_score = [], [], [], []
            for _ in range(rounds):
                for G in groups:
                    t0 = time.perf_counter()
                    aspace.search_fused(G, gl, TAU, subset=sub)
                    t1 = time.perf_counter()
                    aspace.score_fused(G, gl, TAU, ids)
                    t2 = time.perf_counter()
                    F = fused_ref.fuse(aspace.score_items_batch(G, gl, TAU, ids), w, "sum")
                    t3 = time.perf_counter()
                    fused_ref.top(ids, F, topk)
                    t4 = time.perf_counter()
                    t_search.append((t1 - t0) * 1e6)
                    t_score.append((t2 - t1) * 1e6)
                    b_score.append((t3 - t2) * 1e6)
                    b_search.append((t4 - t2) * 1e6)
            ks = []
            assert L.as_set_tuning(b"fused_timing", 1) == 0
            try:
                for G in groups:
                    aspace.search_fused(G, gl, TAU, subset=sub)
                    ks.append(L.as_fused_kernel_us(aspace._h))
            finally:
                assert L.as_set_tuning(b"fused_timing", 0) == 0
            missed = [form for form, new, old in (("search_fused", t_search, b_search), ("score_fused", t_score, b_score)) if med(new) > med(old)]
            verdict = "" if not missed else " -- SLOWER THAN THE BASELINE: " + ", ".join(missed)
            if missed and m >= 100_000:
                worse.append(f"J={J} M={m} ({', '.join(missed)})")
            mb = J * m * 8 / 1e6
            lines.append(f"J={J} M={m}: search_fused median {med(t_search):.1f} us | baseline median {med(b_search):.1f} us | ratio "
                         f"{med(b_search) / med(t_search):.2f}x || score_fused median {med(t_score):.1f} us | baseline median {med(b_score):.1f} us | "
                         f"ratio {med(b_score) / med(t_score):.2f}x || accumulate kernel median {med(ks):.1f} us min {min(ks):.1f} us "
                         f"({mb:.2f} MB of scores, {mb * 1e3 / max(med(ks), 1e-9):.1f} GB/s at the median){verdict}")
            print(lines[-1], flush=True)
        del sub
    lines.append(f"fused_counters {aspace.fused_counters()}")
    lines.append("every cell with M >= 100 000 at or below its baseline" if not worse
                 else "cells with M >= 100 000 slower than their baseline: " + "; ".join(worse))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
