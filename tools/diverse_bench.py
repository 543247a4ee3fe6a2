"""Diversified search (greedy MMR) at the headline size: `search_diverse` and `search_batch_diverse`
against the only route there was before them -- `search` (`search_batch`), `get_item` once per hit and the greedy in numpy on the
host (tests/diverse_ref.py `mmr_path`, which forms only the (n - 1) P dots the greedy needs) -- alternating in one process, and the
select kernel's own duration by HIP events (as_set_tuning("diverse_timing")).  Blocks have DIV_WAVES x 64 = 1024 threads
(as_diverse.hip); the recorded file also holds 256 threads, from a build that could switch between the two.
python tools/diverse_bench.py [N] [D] [NQ] [ROUNDS] [B] [OUT]  (defaults 1M x 768, 8 queries, 5 rounds, B = 1024,
profiles/r14_diverse.txt).

Data: clustered Gaussians around 1 024 centres, rows normalised, fp32 (torch RNG, seed 42), L2 distance / Gaussian weights,
k = 25, tau = 0.62, eps such that a row has about 2 k items inside it; queries: perturbed items (seed 43).  Cells: topk = 100 (the
pool), n = 10, diversity 0.5: the single form, and B queries in one call; topk = 1 024, n = 15: the large pool.  Every answer is
checked first with the stepwise check of tests/diverse_ref.py against the rows `get_item` returns, and compared with the
baseline's picks.  Reports medians over queries x rounds: `search` alone, the single form and what it adds to `search` (paired
differences), the baseline, the kernel's microseconds and the bytes (n - 1) P Dp 4 it re-reads over that time, and the
per-query time of the batched form against the single form's and the batched baseline's."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import diverse_ref as dr  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, make_queries, med  # noqa: E402

TAU = 0.62
L = asp._L
BLOCK = 1024   # threads of a block of diverse_select_kernel (DIV_WAVES x 64)


def host_rows(aspace, pool):
    """What the host route works on: the pool's rows, one get_item per hit, their squared norms and the scores."""
    Xp = np.stack([aspace.get_item(i)[0] for i, _ in pool])
    return Xp, np.einsum("ij,ij->i", Xp, Xp), np.array([v for _, v in pool])


def host_mmr(aspace, pool, n, delta):
    Xp, n64, s = host_rows(aspace, pool)
    picks, margins, _ = dr.mmr_path(Xp, n64, np.arange(len(pool)), s, n, delta)
    return [(pool[p][0], pool[p][1], m) for p, m in zip(picks, margins)]


def check(aspace, res, pool, delta, tol):
    """The stepwise check of an answer against its pool (pool positions stand for the ids: the rows are the gathered ones)."""
    Xp, n64, s = host_rows(aspace, pool)
    pos = {i: p for p, (i, _) in enumerate(pool)}
    assert [v for _, v, _ in res] == [pool[pos[i]][1] for i, _, _ in res]
    return dr.check_steps([(pos[i], v, m) for i, v, m in res], Xp, n64, np.arange(len(pool)), s, delta, tol)


def single_cell(aspace, gl, Q, n, delta, rounds, tol, lines, tag):
    d, dp = aspace.nfeatures, -(-aspace.nfeatures // 32) * 32
    P = len(aspace.search(Q[0], gl, TAU))
    amb = same = 0
    for q in Q:   # the answers, and the warm-up
        pool = aspace.search(q, gl, TAU)
        res = aspace.search_diverse(q, gl, TAU, n, delta, with_margins=True)
        amb += check(aspace, res, pool, delta, tol)
        same += [i for i, _, _ in res] == [i for i, _, _ in host_mmr(aspace, pool, n, delta)]
    t_s, t_new, t_old, ks = [], [], [], []
    for _ in range(rounds):
        for q in Q:
            t0 = time.perf_counter()
            aspace.search(q, gl, TAU)
            t1 = time.perf_counter()
            aspace.search_diverse(q, gl, TAU, n, delta)
            t2 = time.perf_counter()
            host_mmr(aspace, aspace.search(q, gl, TAU), n, delta)
            t3 = time.perf_counter()
            t_s.append((t1 - t0) * 1e6)
            t_new.append((t2 - t1) * 1e6)
            t_old.append((t3 - t2) * 1e6)
    assert L.as_set_tuning(b"diverse_timing", 1) == 0
    try:
        for q in Q:
            aspace.search_diverse(q, gl, TAU, n, delta)
            ks.append(L.as_diverse_kernel_us(aspace._h))
    finally:
        assert L.as_set_tuning(b"diverse_timing", 0) == 0
    added = med(np.array(t_new) - np.array(t_s))
    nbytes = (min(n, P) - 1) * P * dp * 4
    lines.append(f"{tag} single, block {BLOCK}: search {med(t_s):.1f} us | search_diverse {med(t_new):.1f} us (adds {added:.1f} us to search) | "
                 f"baseline (search + {P} get_item + numpy greedy) {med(t_old):.1f} us | ratio {med(t_old) / med(t_new):.1f}x | select kernel "
                 f"median {med(ks):.1f} us min {min(ks):.1f} us, {nbytes / 1e6:.2f} MB re-read = {nbytes / med(ks) / 1e3:.1f} GB/s")
    print(lines[-1], flush=True)
    lines.append(f"{tag} single: {len(Q)} answers pass the stepwise check ({amb} ambiguous steps), {same} equal the baseline's picks; D={d} P={P} n={n}")
    return med(t_new), med(t_old), med(t_s), added


def batch_cell(aspace, gl, Qb, n, delta, rounds, tol, lines, tag, with_baseline):
    b = Qb.shape[0]
    pools = aspace.search_batch(Qb, gl, TAU)
    got = aspace.search_batch_diverse(Qb, gl, TAU, n, delta, with_margins=True)
    amb = sum(check(aspace, g, p, delta, tol) for g, p in zip(got, pools))
    lines.append(f"{tag} B={b}: every answer passes the stepwise check against search_batch's pool ({amb} ambiguous steps)")

    def baseline():
        return [host_mmr(aspace, p, n, delta) for p in aspace.search_batch(Qb, gl, TAU)]

    t_s, t_new, t_old = [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        aspace.search_batch(Qb, gl, TAU)
        t1 = time.perf_counter()
        aspace.search_batch_diverse(Qb, gl, TAU, n, delta)
        t2 = time.perf_counter()
        if with_baseline:
            baseline()
        t3 = time.perf_counter()
        t_s.append((t1 - t0) * 1e6 / b)
        t_new.append((t2 - t1) * 1e6 / b)
        t_old.append((t3 - t2) * 1e6 / b)
    assert L.as_set_tuning(b"diverse_timing", 1) == 0
    try:
        aspace.search_batch_diverse(Qb, gl, TAU, n, delta)
        ku = L.as_diverse_kernel_us(aspace._h)
    finally:
        assert L.as_set_tuning(b"diverse_timing", 0) == 0
    base = f"baseline (search_batch + get_item per hit + numpy greedy) {med(t_old):.1f} us | ratio {med(t_old) / med(t_new):.1f}x | " if with_baseline else ""
    lines.append(f"{tag} B={b}, block {BLOCK}, per query: search_batch {med(t_s):.1f} us | search_batch_diverse {med(t_new):.1f} us | {base}"
                 f"select kernel {ku:.1f} us for the call = {ku / b:.2f} us per query")
    print(lines[-1], flush=True)
    return med(t_new), med(t_old), med(t_s)


def main():
    argv = sys.argv[1:]
    n_items = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    nq = int(argv[2]) if len(argv) > 2 else 8
    rounds = int(argv[3]) if len(argv) > 3 else 5
    b = int(argv[4]) if len(argv) > 4 else 1024
    out = argv[5] if len(argv) > 5 else os.path.join(ROOT, "profiles", "r14_diverse.txt")
    X = gpu_clustered(n_items, d, 42)
    eps = calibrate_eps(X, 25)
    Q = make_queries(X, max(nq, b), 43)
    tol = dr.tol_for(d)
    lines = [f"search_diverse / search_batch_diverse vs search + get_item per hit + numpy greedy: N={n_items} D={d} k=25 l2/gaussian eps={eps:.5f} "
             f"tau={TAU}, {nq} queries x {rounds} rounds alternating; kernel = diverse_select_kernel by HIP events (separate pass)"]
    gp = {"eps": eps, "k": 25, "topk": 100, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n_items, d, d)
    torch.cuda.synchronize()
    s_new, s_old, s_search, s_added = single_cell(aspace, gl, Q[:nq], 10, 0.5, rounds, tol, lines, "topk=100 n=10 delta=0.5")
    b_new, b_old, _ = batch_cell(aspace, gl, np.ascontiguousarray(Q[:b]), 10, 0.5, max(rounds // 2, 2), tol, lines, "topk=100 n=10 delta=0.5", True)
    lines.append(f"diverse_counters {aspace.diverse_counters()}")
    del aspace, gl
    gp = dict(gp, topk=1024)
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n_items, d, d)
    torch.cuda.synchronize()
    single_cell(aspace, gl, Q[:nq], 15, 0.5, max(rounds // 2, 2), tol, lines, "topk=1024 n=15 delta=0.5 (the large pool)")
    batch_cell(aspace, gl, np.ascontiguousarray(Q[:min(b, 256)]), 15, 0.5, 2, tol, lines, "topk=1024 n=15 delta=0.5 (the large pool)", False)
    lines.append(f"both forms beat their baseline's median: single {'yes' if s_new < s_old else 'NO'} ({s_new:.1f} vs {s_old:.1f} us), batched "
                 f"{'yes' if b_new < b_old else 'NO'} ({b_new:.1f} vs {b_old:.1f} us per query)")
    lines.append(f"the batched form's per-query time is below the single form's: {'yes' if b_new < s_new else 'NO'} ({b_new:.1f} vs {s_new:.1f} us)")
    lines.append(f"the single form adds {s_added:.1f} us to a search of {s_search:.1f} us" + (": MORE than the search itself" if s_added > s_search else ""))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
