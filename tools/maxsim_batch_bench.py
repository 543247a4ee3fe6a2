"""Batched late-interaction search at the headline size: `search_maxsim_batch` / `score_maxsim_batch` against the route there was
before them -- the loop of `search_maxsim` / `score_maxsim` calls over the same needs -- alternating in one process, and the
durations of pass A and of the segmented fold kernel by HIP events (as_set_tuning("maxsim_batch_timing")).
python tools/maxsim_batch_bench.py [N] [D] [ROUNDS] [OUT] [CELLS] [RECIPES]  (defaults 1M x 768, 5 rounds,
profiles/r19_maxsim_batch.txt, CELLS = 8x8,8x32,64x8,64x32,256x8 as BxJ, RECIPES = a,b,c; comma-separated, to split a run).

Data: tools/maxsim_bench.py's (clustered Gaussians, fp32, L2 / Gaussian, k = 25, topk = 15, tau = 0.62; query vectors: perturbed
items, seed 43), weights 1/J_b, n_groups = 10, over its three recipes: (a) all N items in N / 10 contiguous groups of 10, (b) all N
items under 1 000 random labels, (c) M = N / 10 items that form N / 100 of the contiguous groups, the re-ranking case.  Every
cell's answers are checked before it is timed: `score_maxsim_batch` over a sample of whole groups against `score_items_batch` of
the call's flattened vectors over those groups' members, folded by tests/maxsim_batch_ref.py (score bits), and every need's list
against tests/maxsim_ref.py's order of its row of `score_maxsim_batch` over every label (labels and score bits).  Reports the
medians over the rounds of one batched call and of one loop over the B needs, both PER NEED, with min - max, the ratio, and the
event times of one call (a separate pass) with the bytes moved and TB/s against the 8 TB/s peak."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import maxsim_batch_ref  # noqa: E402
import maxsim_ref  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, make_queries, med  # noqa: E402

TAU = 0.62
NG = 10
CELLS = ((8, 8), (8, 32), (64, 8), (64, 32), (256, 8))
SAMPLE_IDS = 4096          # members of the sampled groups of the reference check, about
PEAK_TBS = 8.0


def span(x):
    return f"median {med(x):.1f} us ({min(x):.1f} - {max(x):.1f})"


def check_cell(aspace, gl, needs, grp, labels, ids, sub, rng):
    """The score form over a sample of whole groups against the reference; every need's list against its row of scores."""
    B, J = needs.shape[0], needs.shape[1]
    V = np.ascontiguousarray(needs.reshape(B * J, -1))
    offs = np.arange(B + 1) * J
    w = maxsim_batch_ref.default_weights(offs)
    lab_of_ids = labels[ids]
    every = np.unique(lab_of_ids)
    take = max(1, min(len(every), SAMPLE_IDS * len(every) // len(ids)))
    some = np.sort(rng.choice(every, take, replace=False))
    members = ids[np.isin(lab_of_ids, some)]
    S = aspace.score_items_batch(V, gl, TAU, members)
    lab, F = maxsim_batch_ref.maxsim_batch(S, labels[members], offs, w)
    assert lab.tolist() == some.tolist()
    assert aspace.score_maxsim_batch(needs, gl, TAU, grp, some, subset=sub).tobytes() == F.tobytes()
    rows = aspace.score_maxsim_batch(needs, gl, TAU, grp, every, subset=sub)
    hits = aspace.search_maxsim_batch(needs, gl, TAU, grp, NG, subset=sub)
    for b in range(B):
        wl, wf = maxsim_ref.top(every, rows[b], NG)
        assert [l for l, _ in hits[b]] == wl.tolist(), (b, hits[b], wl)
        assert np.array([v for _, v in hits[b]]).tobytes() == wf.tobytes()
    return every


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    rounds = int(argv[2]) if len(argv) > 2 else 5
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r19_maxsim_batch.txt")
    cells = tuple(tuple(int(v) for v in c.split("x")) for c in argv[4].split(",")) if len(argv) > 4 else CELLS
    want = tuple(argv[5].split(",")) if len(argv) > 5 else ("a", "b", "c")
    X = gpu_clustered(n, d, 42)
    gp = {"eps": calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = make_queries(X, max(B * J for B, J in cells), 43)
    del X
    torch.cuda.synchronize()
    L = asp._L
    rng = np.random.default_rng(44)
    by_ten = np.arange(n, dtype=np.int64) // 10
    chosen = np.sort(rng.choice(by_ten[-1] + 1, max((by_ten[-1] + 1) // 10, 1), replace=False))
    recipes = (("a", "all N, contiguous groups of 10", by_ten, None),
               ("b", "all N, 1 000 random labels", rng.integers(0, 1000, n), None),
               ("c", "re-ranking: a tenth of the contiguous groups", by_ten, np.flatnonzero(np.isin(by_ten, chosen))))
    lines = [f"search_maxsim_batch / score_maxsim_batch vs the loop of search_maxsim / score_maxsim over the same needs: N={n} D={d} k=25 "
             f"topk={gp['topk']} l2/gaussian eps={gp['eps']:.5f} tau={TAU}, weights 1/J, n_groups={NG}, {rounds} rounds alternating, medians "
             f"PER NEED (one call or one loop, divided by B) with min - max; kernels by HIP events over one batched search call (separate "
             f"pass): pass A with the memset of its cells over nv*M*16 bytes read (scores, ids, group numbers) + nv*G*8 zeroed, and "
             f"maxsim_fold_batch_kernel over nv*G*8 bytes of cells read + the accumulator rows it writes (and reads when carried) per "
             f"chunk, TB/s against the {PEAK_TBS:.0f} TB/s peak"]
    missed = []
    for key, cname, labels, ids in recipes:
        if key not in want:
            continue
        grp = aspace.groups(labels)
        G = grp.ngroups
        sub = None if ids is None else aspace.subset(ids)
        ids = np.arange(n) if ids is None else ids
        m = len(ids)
        for B, J in cells:
            needs = np.ascontiguousarray(Q[:B * J].reshape(B, J, d))
            listed = check_cell(aspace, gl, needs, grp, labels, ids, sub, rng)[:1000]   # the answers, and the warm-up
            for V in needs:
                aspace.search_maxsim(V, gl, TAU, grp, NG, subset=sub)
                aspace.score_maxsim(V, gl, TAU, grp, listed, subset=sub)
            t_search, t_score, l_search, l_score = [], [], [], []
            for _ in range(rounds):
                t0 = time.perf_counter()
                aspace.search_maxsim_batch(needs, gl, TAU, grp, NG, subset=sub)
                t1 = time.perf_counter()
                for V in needs:
                    aspace.search_maxsim(V, gl, TAU, grp, NG, subset=sub)
                t2 = time.perf_counter()
                aspace.score_maxsim_batch(needs, gl, TAU, grp, listed, subset=sub)
                t3 = time.perf_counter()
                for V in needs:
                    aspace.score_maxsim(V, gl, TAU, grp, listed, subset=sub)
                t4 = time.perf_counter()
                t_search.append((t1 - t0) * 1e6 / B)
                l_search.append((t2 - t1) * 1e6 / B)
                t_score.append((t3 - t2) * 1e6 / B)
                l_score.append((t4 - t3) * 1e6 / B)
            assert L.as_set_tuning(b"maxsim_batch_timing", 1) == 0
            try:
                c0 = aspace.maxsim_batch_counters()
                aspace.search_maxsim_batch(needs, gl, TAU, grp, NG, subset=sub)
                ka, kf = L.as_maxsim_batch_kernel_us(aspace._h, 1), L.as_maxsim_batch_kernel_us(aspace._h, 2)
                c1 = aspace.maxsim_batch_counters()
            finally:
                assert L.as_set_tuning(b"maxsim_batch_timing", 0) == 0
            dc = {k: c1[k] - c0[k] for k in c1}
            nv = B * J
            bytes_a = nv * m * 16 + nv * G * 8
            bytes_f = nv * G * 8 + (B + dc["fold_launches"]) * G * 8 * 2   # (an upper bound on the accumulator rows written and carried)
            forms = [("search_maxsim_batch", t_search, l_search), ("score_maxsim_batch", t_score, l_score)]
            slow = [f"{form} by {100.0 * (med(new) / med(old) - 1.0):.1f} %" for form, new, old in forms if med(new) > med(old)]
            if slow:
                missed.append(f"B={B} J={J} {cname} ({', '.join(slow)})")
            line = (f"{cname} (M={m}, G={G}), B={B} J={J}: search_maxsim_batch {span(t_search)} per need | loop {span(l_search)} per need | "
                    f"ratio {med(l_search) / med(t_search):.2f}x || score_maxsim_batch ({len(listed)} labels) {span(t_score)} per need | loop "
                    f"{span(l_score)} per need | ratio {med(l_score) / med(t_score):.2f}x || pass A {ka:.1f} us in {dc['pass_a_launches']} "
                    f"launches, {bytes_a / 1e6:.1f} MB, {bytes_a / max(ka, 1e-9) / 1e6:.2f} TB/s ({100.0 * bytes_a / max(ka, 1e-9) / 1e6 / PEAK_TBS:.0f} % "
                    f"of peak), {ka / nv / (m / 1e6):.1f} us per vector and million positions | fold kernel {kf:.1f} us in "
                    f"{dc['fold_launches']} launches, {dc['need_groups']} need group(s), {bytes_f / 1e6:.1f} MB, "
                    f"{bytes_f / max(kf, 1e-9) / 1e6:.2f} TB/s ({100.0 * bytes_f / max(kf, 1e-9) / 1e6 / PEAK_TBS:.0f} % of peak)")
            lines.append(line + (" -- SLOWER THAN THE LOOP: " + ", ".join(slow) if slow else ""))
            print(lines[-1], flush=True)
        del sub, grp
    lines.append(f"maxsim_batch_counters {aspace.maxsim_batch_counters()}")
    lines.append("condition (batched median per need <= the loop's, every cell): met" if not missed
                 else "condition (batched median per need <= the loop's, every cell): MISSED in " + "; ".join(missed))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
