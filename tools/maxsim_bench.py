"""Late-interaction search (MaxSim) at the headline size: `search_maxsim` against the only exact route there was before it --
`score_items_batch` of the J vectors over the ids (a J x M matrix of fp64 scores to host memory), then the numpy group-by, fold
and order of tests/maxsim_ref.py -- and against `search_fused` over the same ids, which has the same gather and the same
selection, so that the difference is what the group maxima cost.  The three routes alternate per need in one process; the pass-A
and fold kernels are timed by HIP events in a separate pass (as_set_tuning("maxsim_timing")).
python tools/maxsim_bench.py [N] [D] [NEEDS] [ROUNDS] [OUT]  (defaults 1M x 768, 8 needs, 5 rounds, profiles/r18_maxsim.txt).

Data: tools/fused_bench.py's (clustered Gaussians, fp32, L2 / Gaussian, k = 25, topk = 15, tau = 0.62); a need: J perturbed items
(seed 43), weights 1/J, n_groups = 10.  Cells: J = 8, 32 over (a) all N items in N / 10 contiguous groups of 10, (b) all N items
under 1 000 random labels, (c) M = N / 10 items that form N / 100 of the contiguous groups, the re-ranking case.  Every need's
answer is checked against the baseline's (labels and score bits) before it is timed.  Reports the medians with min - max over
needs x rounds."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import maxsim_ref  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, make_queries, med  # noqa: E402

TAU = 0.62
JS = (8, 32)
NG = 10


def span(x):
    return f"median {med(x):.1f} us ({min(x):.1f} - {max(x):.1f})"


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    needs = int(argv[2]) if len(argv) > 2 else 8
    rounds = int(argv[3]) if len(argv) > 3 else 5
    out = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "r18_maxsim.txt")
    X = gpu_clustered(n, d, 42)
    gp = {"eps": calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = make_queries(X, needs * max(JS), 43)
    del X
    torch.cuda.synchronize()
    L = asp._L
    rng = np.random.default_rng(44)
    by_ten = np.arange(n, dtype=np.int64) // 10
    chosen = np.sort(rng.choice(by_ten[-1] + 1, max((by_ten[-1] + 1) // 10, 1), replace=False))
    cells = (("all N, contiguous groups of 10", by_ten, None),
             ("all N, 1 000 random labels", rng.integers(0, 1000, n), None),
             ("re-ranking: a tenth of the contiguous groups", by_ten, np.flatnonzero(np.isin(by_ten, chosen))))
    lines = [f"search_maxsim vs score_items_batch + numpy group-by, fold and order (maxsim_ref) vs search_fused over the same ids: N={n} D={d} "
             f"k=25 topk={gp['topk']} l2/gaussian eps={gp['eps']:.5f} tau={TAU}, weights 1/J, n_groups={NG}, {needs} needs x {rounds} rounds "
             f"alternating; kernels by HIP events (separate pass): pass A with the memset of its cells, and maxsim_fold_kernel with GB/s over "
             f"the J*G*8 bytes of cells it reads plus the G*8 it writes per chunk"]
    worse = []
    for cname, labels, ids in cells:
        grp = aspace.groups(labels)
        G = grp.ngroups
        sub = None if ids is None else aspace.subset(ids)
        ids = np.arange(n) if ids is None else ids
        lab_of_ids = labels[ids]
        for J in JS:
            vecs = [np.ascontiguousarray(Q[g * J:(g + 1) * J]) for g in range(needs)]
            w = np.full(J, 1.0 / J)

            def baseline(V):
                lab, F = maxsim_ref.maxsim(aspace.score_items_batch(V, gl, TAU, ids), lab_of_ids, w)
                return maxsim_ref.top(lab, F, NG)

            for V in vecs:   # the answers, and the warm-up
                wl, wf = baseline(V)
                got = aspace.search_maxsim(V, gl, TAU, grp, NG, subset=sub)
                assert [l for l, _ in got] == wl.tolist(), (got, wl)
                assert np.array([v for _, v in got]).tobytes() == wf.tobytes()
                aspace.search_fused(V, gl, TAU, subset=sub)
            t_new, t_old, t_fused = [], [], []
            for _ in range(rounds):
                for V in vecs:
                    t0 = time.perf_counter()
                    aspace.search_maxsim(V, gl, TAU, grp, NG, subset=sub)
                    t1 = time.perf_counter()
                    baseline(V)
                    t2 = time.perf_counter()
                    aspace.search_fused(V, gl, TAU, subset=sub)
                    t3 = time.perf_counter()
                    t_new.append((t1 - t0) * 1e6)
                    t_old.append((t2 - t1) * 1e6)
                    t_fused.append((t3 - t2) * 1e6)
            ka, kf = [], []
            c0 = aspace.maxsim_counters()
            assert L.as_set_tuning(b"maxsim_timing", 1) == 0
            try:
                for V in vecs:
                    aspace.search_maxsim(V, gl, TAU, grp, NG, subset=sub)
                    ka.append(L.as_maxsim_kernel_us(aspace._h, 1))
                    kf.append(L.as_maxsim_kernel_us(aspace._h, 2))
            finally:
                assert L.as_set_tuning(b"maxsim_timing", 0) == 0
            c1 = aspace.maxsim_counters()
            chunks = (c1["fold_launches"] - c0["fold_launches"]) // needs
            atoms = (c1["max_atomics"] - c0["max_atomics"]) / (needs * J)
            mb = (J * G * 8 + chunks * G * 8) / 1e6
            slower = med(t_new) > med(t_old)
            if slower:
                worse.append(f"J={J}, {cname}")
            lines.append(f"{cname} (M={len(ids)}, G={G}), J={J}: search_maxsim {span(t_new)} | baseline {span(t_old)} | ratio "
                         f"{med(t_old) / med(t_new):.2f}x | search_fused {span(t_fused)}, the group maxima cost {med(t_new) - med(t_fused):+.1f} us || "
                         f"pass A {span(ka)}, {atoms:.0f} max-atomics per vector | fold kernel {span(kf)}, {chunks} chunk(s), {mb:.3f} MB, "
                         f"{mb * 1e3 / max(med(kf), 1e-9):.1f} GB/s at the median{' -- SLOWER THAN THE BASELINE' if slower else ''}")
            print(lines[-1], flush=True)
        del sub, grp
    lines.append(f"maxsim_counters {aspace.maxsim_counters()}")
    lines.append("every cell at or below its baseline" if not worse else "cells slower than their baseline: " + "; ".join(worse))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
