"""Late-interaction re-ranking of per-need candidate documents at the headline size: `search_maxsim_lists` against the two routes
there were before it, alternating in one process -- (i) the loop of `search_maxsim(need_b, ..., subset=members of b's candidates)`,
one subset per need, and (ii) `score_lists_batch` over the flattened vectors, each with its need's expanded id list, followed by
the numpy group-by of tests/maxsim_lists_ref.py -- and the durations of the new score kernel, fold kernel and selection by HIP
events (as_set_tuning("maxsim_lists_timing")) beside `lists_score_kernel`'s over the J-times repeated lists ("lists_timing").
python tools/maxsim_lists_bench.py [N] [D] [ROUNDS] [OUT] [CELLS] [CANDS]  (defaults 1M x 768, 5 rounds,
profiles/r20_maxsim_lists.txt, CELLS = 64x8,64x32,256x8,1024x8 as BxJ, CANDS = 100,1000,ragged; comma-separated, to split a run).

Data: tools/maxsim_bench.py's (clustered Gaussians, fp32, L2 / Gaussian, k = 25, topk = 15, tau = 0.62; query vectors: perturbed
items, seed 43), weights 1/J, n_groups = 10, all N items in N / 10 contiguous groups of 10; candidates per need: 100 or 1 000
random documents, or one ragged draw of 10 .. 1 000.  Every cell's answers are checked before it is timed: every need's list
against tests/maxsim_lists_ref.py over route (ii)'s scores (labels and score bits).  Reports the medians over the rounds PER NEED
with min - max, the ratios, the event times of one call (a separate pass) with the gather rate of the score kernel (rows asked for
x D x 4 bytes) against the 8 TB/s peak, and the shares of the fold, the selection and the host preparation in a call."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import maxsim_lists_ref  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, make_queries, med  # noqa: E402

TAU = 0.62
NG = 10
CELLS = ((64, 8), (64, 32), (256, 8), (1024, 8))
CANDS = ("100", "1000", "ragged")
PEAK_TBS = 8.0


def span(x):
    return f"median {med(x):.1f} us ({min(x):.1f} - {max(x):.1f})"


def route_two(aspace, gl, V, J, ids, labels):
    """Route (ii): the scores of every (vector, entry) pair on the host, then the numpy group-by, fold and order."""
    rows = aspace.score_lists_batch(V, gl, TAU, [ids[v // J] for v in range(V.shape[0])])
    S = [np.stack(rows[b * J:(b + 1) * J]) for b in range(len(ids))]
    per = maxsim_lists_ref.maxsim_lists(S, [labels[i] for i in ids], maxsim_lists_ref.default_weights([J] * len(ids)))
    return maxsim_lists_ref.top_lists(per, NG)


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    rounds = int(argv[2]) if len(argv) > 2 else 5
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r20_maxsim_lists.txt")
    cells = tuple(tuple(int(v) for v in c.split("x")) for c in argv[4].split(",")) if len(argv) > 4 else CELLS
    cands = tuple(argv[5].split(",")) if len(argv) > 5 else CANDS
    X = gpu_clustered(n, d, 42)
    gp = {"eps": calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = make_queries(X, max(B * J for B, J in cells), 43)
    del X
    torch.cuda.synchronize()
    L = asp._L
    rng = np.random.default_rng(45)
    assert n % 10 == 0 and n >= 10_000, "contiguous groups of 10, at least 1 000 of them"
    labels = np.arange(n, dtype=np.int64) // 10
    G = int(labels[-1]) + 1
    grp = aspace.groups(labels)
    geo = aspace.maxsim_lists_geometry()
    lines = [f"search_maxsim_lists vs (i) the loop of search_maxsim with one subset per need and (ii) score_lists_batch over the J-times "
             f"repeated lists + the numpy group-by: N={n} D={d} k=25 topk={gp['topk']} l2/gaussian eps={gp['eps']:.5f} tau={TAU}, weights 1/J, "
             f"n_groups={NG}, {G} contiguous groups of 10, tile={geo['tile']} vectors, segment={geo['segment']} entries, {rounds} rounds "
             f"alternating, medians PER NEED (one call or one loop, divided by B) with min - max; kernels by HIP events over one call "
             f"(separate pass); gather rate = rows asked for x D x 4 bytes over the score kernel's time against the {PEAK_TBS:.0f} TB/s peak"]
    missed, kernel_missed = [], []
    for B, J in cells:
        needs = np.ascontiguousarray(Q[:B * J].reshape(B, J, d))
        V = np.ascontiguousarray(needs.reshape(B * J, d))
        for cand in cands:
            counts = rng.integers(10, 1001, B) if cand == "ragged" else np.full(B, int(cand))
            lists = [np.sort(rng.choice(G, int(c), replace=False)) for c in counts]
            ids = [(l[:, None] * 10 + np.arange(10)[None, :]).reshape(-1) for l in lists]   # (label, item id) order: contiguous groups of 10
            # the answers (and the warm-up of all three routes)
            want = route_two(aspace, gl, V, J, ids, labels)
            hits = aspace.search_maxsim_lists(needs, gl, TAU, grp, NG, lists)
            for b in range(B):
                assert [l for l, _ in hits[b]] == want[b][0].tolist(), (b, hits[b], want[b])
                assert np.array([v for _, v in hits[b]]).tobytes() == want[b][1].tobytes(), b
            aspace.search_maxsim(needs[0], gl, TAU, grp, NG, subset=aspace.subset(ids[0]))
            t_new, t_loop, t_two = [], [], []
            c0 = aspace.maxsim_lists_counters()
            for _ in range(rounds):
                t0 = time.perf_counter()
                aspace.search_maxsim_lists(needs, gl, TAU, grp, NG, lists)
                t1 = time.perf_counter()
                for b in range(B):
                    aspace.search_maxsim(needs[b], gl, TAU, grp, NG, subset=aspace.subset(ids[b]))
                t2 = time.perf_counter()
                route_two(aspace, gl, V, J, ids, labels)
                t3 = time.perf_counter()
                t_new.append((t1 - t0) * 1e6 / B)
                t_loop.append((t2 - t1) * 1e6 / B)
                t_two.append((t3 - t2) * 1e6 / B)
            c1 = aspace.maxsim_lists_counters()
            host_share = (c1["host_ns"] - c0["host_ns"]) / 1e3 / rounds / B / med(t_new)
            assert L.as_set_tuning(b"maxsim_lists_timing", 1) == 0 and L.as_set_tuning(b"lists_timing", 1) == 0
            try:
                c0 = aspace.maxsim_lists_counters()
                aspace.search_maxsim_lists(needs, gl, TAU, grp, NG, lists)
                ks, kf, kx = (L.as_maxsim_lists_kernel_us(aspace._h, p) for p in (1, 2, 3))
                c1 = aspace.maxsim_lists_counters()
                aspace.score_lists_batch(V, gl, TAU, [ids[v // J] for v in range(B * J)])
                kl = L.as_lists_kernel_us(aspace._h)
            finally:
                assert L.as_set_tuning(b"maxsim_lists_timing", 0) == 0 and L.as_set_tuning(b"lists_timing", 0) == 0
            dc = {k: c1[k] - c0[k] for k in c1}
            gathered = dc["row_reads"] * d * 4
            call_us = med(t_new) * B
            slow = [f"route ({r}) by {100.0 * (med(t_new) / med(old) - 1.0):.1f} % (its spread {max(old) - min(old):.1f} us)"
                    for r, old in (("i", t_loop), ("ii", t_two)) if med(old) - med(t_new) <= max(old) - min(old)]
            if slow:
                missed.append(f"B={B} J={J} candidates={cand} ({', '.join(slow)})")
            if ks >= kl:
                kernel_missed.append(f"B={B} J={J} candidates={cand} ({ks:.1f} us against {kl:.1f} us)")
            line = (f"B={B} J={J} candidates={cand} ({int(counts.sum())} documents, {dc['row_reads']} rows asked for, {dc['pairs']} dots): "
                    f"search_maxsim_lists {span(t_new)} per need | (i) loop of search_maxsim {span(t_loop)} per need, ratio "
                    f"{med(t_loop) / med(t_new):.2f}x | (ii) score_lists_batch + numpy {span(t_two)} per need, ratio {med(t_two) / med(t_new):.2f}x || "
                    f"score kernel {ks:.1f} us in {dc['score_launches']} launches against lists_score_kernel {kl:.1f} us over the repeated lists "
                    f"({kl / max(ks, 1e-9):.2f}x), {gathered / 1e6:.1f} MB gathered, {gathered / max(ks, 1e-9) / 1e6:.2f} TB/s "
                    f"({100.0 * gathered / max(ks, 1e-9) / 1e6 / PEAK_TBS:.0f} % of peak) | fold {kf:.1f} us ({100.0 * kf / call_us:.1f} % of a call) | "
                    f"selection {kx:.1f} us ({100.0 * kx / call_us:.1f} %) | host preparation {100.0 * host_share:.1f} % of a call")
            lines.append(line + (" -- NOT BELOW BY MORE THAN THE BASELINE'S SPREAD: " + ", ".join(slow) if slow else ""))
            print(lines[-1], flush=True)
    lines.append(f"maxsim_lists_counters {aspace.maxsim_lists_counters()}")
    lines.append("condition (the new call's median below both routes' by more than the baseline's spread, every cell): met" if not missed
                 else "condition (the new call's median below both routes' by more than the baseline's spread, every cell): MISSED in " + "; ".join(missed))
    lines.append("condition (the score kernel below lists_score_kernel over the repeated lists, every cell): met" if not kernel_missed
                 else "condition (the score kernel below lists_score_kernel over the repeated lists, every cell): MISSED in " + "; ".join(kernel_missed))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
