"""Batched fused search at the headline size: `search_fused_batch` / `score_fused_batch` against the route there was before them --
the loop of `search_fused` / `score_fused` calls over the same needs -- alternating in one process, and the segmented accumulate
kernel's own duration by HIP events (as_set_tuning("fused_batch_timing")).
python tools/fused_batch_bench.py [N] [D] [ROUNDS] [OUT] [BS] [MS]  (defaults 1M x 768, 5 rounds, profiles/r17_fused_batch.txt,
BS = 8,64,256 needs, MS = 1000,100000,N candidates; BS / MS: comma-separated, to split a run).

Data: tools/fused_bench.py's (clustered Gaussians around 1 024 centres, rows normalised, fp32, seed 42, L2 / Gaussian, k = 25,
topk = 15, tau = 0.62, eps such that a row has about 2 k items inside it; query vectors: perturbed items, seed 43), weights 1/J,
mode sum timed.  Cells: B = 8, 64, 256 needs x J = 2, 8 vectors each x a prepared subset of M = 1 000 and 100 000 uniformly
random items and all N (subset=None).  Every cell's answers are checked in both modes before it is timed: `score_fused_batch`
against `score_items_batch` of the call's flattened vectors folded need by need by tests/fused_batch_ref.py (score bits; over
all M ids where that matrix stays under 256 MB, over a sorted sample of 4 096 of them otherwise), and every need's list against
the lexsort of its row of fused scores (indices and score bits; the row is `score_fused_batch`'s where B x M doubles stay under
1 GiB, the single `score_fused`'s of that need otherwise).  The score form is not timed where its answer exceeds 1 GiB.
Reports the medians over the rounds of one batched call and of one loop over the B needs, both per need, the ratio, the
accumulate kernel's microseconds in one call (a separate pass with the events on) and its share of the batched search call."""
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
from fused_batch_ref import default_weights, fuse_batch  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, make_queries, med  # noqa: E402

TAU = 0.62
JS = (2, 8)
FULL_REFERENCE_BYTES = 256 << 20
FULL_ROWS_BYTES = 1 << 30


def same_hits(got, ids, F, k):
    wi, ws = fused_ref.top(ids, F, k)
    assert [i for i, _ in got] == wi.tolist(), (len(got), len(wi))
    assert np.array([v for _, v in got]).tobytes() == ws.tobytes()


def check_cell(aspace, gl, needs, ids, sub, topk, rng):
    """Both modes: the score form against the reference, every need's list against its row of fused scores."""
    B, J = needs.shape[0], needs.shape[1]
    V = np.ascontiguousarray(needs.reshape(B * J, -1))
    offs = np.arange(B + 1) * J
    w = default_weights(offs)
    m = len(ids)
    some = ids if B * J * m * 8 <= FULL_REFERENCE_BYTES else np.sort(rng.choice(ids, 4096, replace=False))
    S = aspace.score_items_batch(V, gl, TAU, some)
    for mode in ("sum", "max"):
        F = fuse_batch(S, offs, w, mode)
        assert aspace.score_fused_batch(needs, gl, TAU, some, mode=mode).tobytes() == F.tobytes()
        hits = aspace.search_fused_batch(needs, gl, TAU, mode=mode, subset=sub)
        if some is not ids:
            F = aspace.score_fused_batch(needs, gl, TAU, ids, mode=mode) if B * m * 8 <= FULL_ROWS_BYTES else None
        for b in range(B):
            same_hits(hits[b], ids, F[b] if F is not None else aspace.score_fused(needs[b], gl, TAU, ids, mode=mode), topk)
        del F


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    rounds = int(argv[2]) if len(argv) > 2 else 5
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r17_fused_batch.txt")
    bs = tuple(int(x) for x in argv[4].split(",")) if len(argv) > 4 else (8, 64, 256)
    ms = tuple(min(int(x), n) for x in argv[5].split(",")) if len(argv) > 5 else (min(1_000, n), min(100_000, n), n)
    X = gpu_clustered(n, d, 42)
    gp = {"eps": calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = make_queries(X, max(bs) * max(JS), 43)
    del X
    torch.cuda.synchronize()
    L = asp._L
    topk = gp["topk"]
    rng = np.random.default_rng(44)
    lines = [f"search_fused_batch / score_fused_batch vs the loop of search_fused / score_fused over the same needs: N={n} D={d} k=25 "
             f"topk={topk} l2/gaussian eps={gp['eps']:.5f} tau={TAU}, weights 1/J, mode sum, {rounds} rounds alternating, medians PER "
             f"NEED (one call or one loop, divided by B); kernel = fused_accumulate_batch_kernel by HIP events, summed over one call "
             f"(separate pass), share = of the batched search call"]
    missed = []
    for m in sorted(set(ms)):
        ids = np.arange(n) if m == n else np.sort(rng.choice(n, m, replace=False))
        sub = None if m == n else aspace.subset(ids)
        for B in bs:
            for J in JS:
                needs = np.ascontiguousarray(Q[:B * J].reshape(B, J, d))
                check_cell(aspace, gl, needs, ids, sub, topk, rng)   # the answers, and the warm-up
                for G in needs:
                    aspace.search_fused(G, gl, TAU, subset=sub)
                score = B * m * 8 <= FULL_ROWS_BYTES
                t_search, t_score, l_search, l_score = [], [], [], []
                for _ in range(rounds):
                    t0 = time.perf_counter()
                    aspace.search_fused_batch(needs, gl, TAU, subset=sub)
                    t1 = time.perf_counter()
                    for G in needs:
                        aspace.search_fused(G, gl, TAU, subset=sub)
                    t2 = time.perf_counter()
                    t_search.append((t1 - t0) * 1e6 / B)
                    l_search.append((t2 - t1) * 1e6 / B)
                    if score:
                        t0 = time.perf_counter()
                        aspace.score_fused_batch(needs, gl, TAU, ids)
                        t1 = time.perf_counter()
                        for G in needs:
                            aspace.score_fused(G, gl, TAU, ids)
                        t2 = time.perf_counter()
                        t_score.append((t1 - t0) * 1e6 / B)
                        l_score.append((t2 - t1) * 1e6 / B)
                assert L.as_set_tuning(b"fused_batch_timing", 1) == 0
                try:
                    c0 = aspace.fused_batch_counters()
                    aspace.search_fused_batch(needs, gl, TAU, subset=sub)
                    kus = L.as_fused_batch_kernel_us(aspace._h)
                    c1 = aspace.fused_batch_counters()
                finally:
                    assert L.as_set_tuning(b"fused_batch_timing", 0) == 0
                forms = [("search_fused_batch", t_search, l_search)] + ([("score_fused_batch", t_score, l_score)] if score else [])
                slow = [f"{form} by {100.0 * (med(new) / med(old) - 1.0):.1f} %" for form, new, old in forms if med(new) > med(old)]
                if slow:
                    missed.append(f"B={B} J={J} M={m} ({', '.join(slow)})")
                line = (f"B={B} J={J} M={m}: search_fused_batch {med(t_search):.1f} us/need | loop {med(l_search):.1f} us/need | ratio "
                        f"{med(l_search) / med(t_search):.2f}x || ")
                line += (f"score_fused_batch {med(t_score):.1f} us/need | loop {med(l_score):.1f} us/need | ratio {med(l_score) / med(t_score):.2f}x || "
                         if score else "score form not timed (its answer exceeds 1 GiB) || ")
                line += (f"accumulate kernel {kus:.1f} us in {c1['launches'] - c0['launches']} launches, {c1['groups'] - c0['groups']} need "
                         f"groups ({100.0 * kus / (med(t_search) * B):.2f} % of the call)")
                lines.append(line + (" -- SLOWER THAN THE LOOP: " + ", ".join(slow) if slow else ""))
                print(lines[-1], flush=True)
        del sub
    lines.append(f"fused_batch_counters {aspace.fused_batch_counters()}")
    lines.append("condition (batched median per need <= the loop's, every cell): met" if not missed
                 else "condition (batched median per need <= the loop's, every cell): MISSED in " + "; ".join(missed))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
