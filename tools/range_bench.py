"""Range search at the headline size: `search_range` against the only route there was before it -- `score_items` of the
subset's ids, a numpy filter and `lexsort` on the host -- per query, alternating in one process, and the compaction kernel's own
duration by HIP events (as_set_tuning("range_timing")).
python tools/range_bench.py [N] [D] [NQ] [ROUNDS] [OUT]  (defaults 1M x 768, 8 queries, 5 rounds, profiles/r13_range.txt).

Data: clustered Gaussians around 1 024 centres, rows normalised, fp32 (torch RNG, seed 42), L2 distance / Gaussian weights,
k = 25, topk = 15, tau = 0.62, eps such that a row has about 2 k items inside it; queries: perturbed items (seed 43).  Cells: a
prepared subset of M = 1 000 and 100 000 uniformly random items and all N (subset=None), each with three thresholds per query
taken from that query's own `score_items` scores so that 0, 100 and 1 % of M survive; and a batched cell, B = 256 queries over
M = 100 000 with 100 survivors each (`search_range_batch` against `score_items_batch` + numpy per row).  Every cell's answer is
checked against the baseline's (indices and score bits) before it is timed.  Reports the medians of both routes over
queries x rounds, the compaction kernel's median microseconds (a separate pass with the events on) and the survivors."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyarrowspace_amd as asp  # noqa: E402

TAU = 0.62
INF = float("inf")


def gpu_clustered(n, d, seed, nclust=1024, noise=0.5, device="cuda"):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    C = torch.randn((nclust, d), generator=g, device=device, dtype=torch.float32)
    z = torch.randint(0, nclust, (n,), generator=g, device=device)
    X = torch.empty((n, d), device=device, dtype=torch.float32)
    for s in range(0, n, 1 << 17):
        e = min(n, s + (1 << 17))
        X[s:e] = C[z[s:e]] + noise * torch.randn((e - s, d), generator=g, device=device, dtype=torch.float32)
        X[s:e] /= X[s:e].norm(dim=1, keepdim=True)
    return X


def calibrate_eps(X, k, sample=512, seed=5):
    """The median over a row sample of the distance to the (2 k)-th nearest item."""
    n = X.shape[0]
    g = torch.Generator(device=X.device)
    g.manual_seed(seed)
    rows = torch.randperm(n, generator=g, device=X.device)[:sample]
    nn = (X * X).sum(1).double()
    D2 = (nn[rows][:, None] + nn[None, :] - 2 * (X[rows] @ X.T).double()).clamp_min(0)
    D2[torch.arange(len(rows), device=X.device), rows] = INF
    kth = int(min(2 * k, n - 1))
    return float(torch.topk(D2, kth, dim=1, largest=False).values[:, -1].median().item()) ** 0.5


def make_queries(X, nq, seed, spread=0.02):
    rng = np.random.default_rng(seed)
    n, d = X.shape
    Q = X[torch.as_tensor(rng.integers(0, n, nq), device=X.device)].double().cpu().numpy() + spread * rng.standard_normal((nq, d)) / np.sqrt(d)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return np.ascontiguousarray(Q)


def filtered(ids, s, thr):
    keep = s >= thr
    i, v = ids[keep], s[keep]
    o = np.lexsort((i, -v))
    return list(zip(i[o].tolist(), v[o].tolist()))


def same(got, want):
    assert [i for i, _ in got] == [i for i, _ in want], (len(got), len(want))
    assert np.array([v for _, v in got]).tobytes() == np.array([v for _, v in want]).tobytes()


def med(x):
    return float(np.median(x))


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    nq = int(argv[2]) if len(argv) > 2 else 8
    rounds = max(int(argv[3]) if len(argv) > 3 else 5, 5)
    out = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "r13_range.txt")
    X = gpu_clustered(n, d, 42)
    gp = {"eps": calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = make_queries(X, max(nq, 256), 43)
    del X
    torch.cuda.synchronize()
    L = asp._L
    rng = np.random.default_rng(44)
    lines = [f"search_range vs score_items + numpy filter + lexsort: N={n} D={d} k=25 topk=15 l2/gaussian eps={gp['eps']:.5f} tau={TAU}, "
             f"{nq} queries x {rounds} rounds alternating, B=1 unless stated; kernel = range_compact_kernel by HIP events (separate pass)"]
    worse = []
    for m in sorted({min(1_000, n), min(100_000, n), n}):
        ids = np.arange(n) if m == n else np.sort(rng.choice(n, m, replace=False))
        sub = None if m == n else aspace.subset(ids)
        scores = [aspace.score_items(q, gl, TAU, ids) for q in Q[:nq]]
        for label, keep in (("0", 0), ("100", min(100, m)), ("1 %", max(m // 100, 1))):
            thr = [float(np.nextafter(s.max(), INF)) if keep == 0 else float(np.sort(s)[::-1][keep - 1]) for s in scores]
            surv = []
            for q, t in zip(Q[:nq], thr):   # the answers, and the warm-up
                got = aspace.search_range(q, gl, TAU, t, sub)
                same(got, filtered(ids, aspace.score_items(q, gl, TAU, ids), t))
                assert aspace.count_range(q, gl, TAU, t, sub) == len(got)
                surv.append(len(got))
            t_new, t_old, t_cnt = [], [], []
            for _ in range(rounds):
                for q, t in zip(Q[:nq], thr):
                    t0 = time.perf_counter()
                    aspace.search_range(q, gl, TAU, t, sub)
                    t1 = time.perf_counter()
                    filtered(ids, aspace.score_items(q, gl, TAU, ids), t)
                    t2 = time.perf_counter()
                    aspace.count_range(q, gl, TAU, t, sub)
                    t3 = time.perf_counter()
                    t_new.append((t1 - t0) * 1e6)
                    t_old.append((t2 - t1) * 1e6)
                    t_cnt.append((t3 - t2) * 1e6)
            ks = []
            assert L.as_set_tuning(b"range_timing", 1) == 0
            try:
                for q, t in zip(Q[:nq], thr):
                    aspace.search_range(q, gl, TAU, t, sub)
                    ks.append(L.as_range_kernel_us(aspace._h))
            finally:
                assert L.as_set_tuning(b"range_timing", 0) == 0
            verdict = "" if med(t_new) <= med(t_old) else " -- SLOWER THAN THE BASELINE"
            if verdict:
                worse.append(f"M={m} survivors {label}")
            lines.append(f"M={m} survivors {label} (median {med(surv):.0f}): search_range median {med(t_new):.1f} us | baseline median "
                         f"{med(t_old):.1f} us | ratio {med(t_old) / med(t_new):.2f}x | count_range median {med(t_cnt):.1f} us | compaction kernel "
                         f"median {med(ks):.1f} us min {min(ks):.1f} us ({m * 8 / 1e6:.2f} MB of scores){verdict}")
            print(lines[-1], flush=True)
        del sub
    # the batched cell
    m, b = min(100_000, n), 256
    ids = np.sort(rng.choice(n, m, replace=False))
    sub = aspace.subset(ids)
    Qb = np.ascontiguousarray(Q[:b])
    S = aspace.score_items_batch(Qb, gl, TAU, ids)
    thr = np.sort(S, axis=1)[:, -min(100, m)].copy()
    del S

    def baseline_batch():
        Sb = aspace.score_items_batch(Qb, gl, TAU, ids)
        return [filtered(ids, Sb[i], thr[i]) for i in range(b)]

    got, want = aspace.search_range_batch(Qb, gl, TAU, thr, sub), baseline_batch()
    for g, w in zip(got, want):
        same(g, w)
    assert aspace.count_range_batch(Qb, gl, TAU, thr, sub).tolist() == [len(g) for g in got]
    t_new, t_old = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        aspace.search_range_batch(Qb, gl, TAU, thr, sub)
        t1 = time.perf_counter()
        baseline_batch()
        t2 = time.perf_counter()
        t_new.append((t1 - t0) * 1e6)
        t_old.append((t2 - t1) * 1e6)
    assert L.as_set_tuning(b"range_timing", 1) == 0
    try:
        aspace.search_range_batch(Qb, gl, TAU, thr, sub)
        ku = L.as_range_kernel_us(aspace._h)
    finally:
        assert L.as_set_tuning(b"range_timing", 0) == 0
    verdict = "" if med(t_new) <= med(t_old) else " -- SLOWER THAN THE BASELINE"
    if verdict:
        worse.append(f"B={b} M={m}")
    lines.append(f"B={b} M={m} survivors 100 per query ({sum(len(g) for g in got)} in all): search_range_batch median {med(t_new):.1f} us | "
                 f"baseline (score_items_batch + numpy per row) median {med(t_old):.1f} us | ratio {med(t_old) / med(t_new):.2f}x | compaction "
                 f"kernel {ku:.1f} us over the call's chunks ({b * m * 8 / 1e6:.1f} MB of scores){verdict}")
    print(lines[-1], flush=True)
    lines.append(f"range_counters {aspace.range_counters()}")
    lines.append("every cell at or below its baseline" if not worse else "cells slower than their baseline: " + "; ".join(worse))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
