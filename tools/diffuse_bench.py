"""Graph-diffusion search at the headline size: `search_diffuse` and `search_batch_diffuse` against
the route there was before them -- `search` (`search_batch`), then the same recurrence on the host over `to_csr()`'s matrix,
prepared once outside the timing (scipy.sparse if importable, else np.add.reduceat) -- alternating in one process, and the step
kernels' own duration by HIP events (as_set_tuning("diffuse_timing")).
python tools/diffuse_bench.py [N] [D] [NQ] [ROUNDS] [OUT]  (defaults 1M x 768, 8 queries, 5 rounds, profiles/r21_diffuse.txt).

Data: clustered Gaussians around 1 024 centres, rows normalised, fp32 (torch RNG, seed 42), L2 distance / Gaussian weights,
k = 25, topk = 100, tau = 0.62, alpha = 0.85, eps such that a row has about 2 k items inside it; queries: perturbed items (seed
43).  Cells: steps 1, 3, 10 x B = 1 (the single form, medians over queries x rounds), B = 64 and B = 1024 (one call per round,
per-query figures).  The batched cells run twice: under "diffuse_mib" = 256 (16 columns per chunk at 1M rows) and
= 1100 (64 columns per chunk, what the default of 1024 MiB gives up to 1M rows).  The host baseline of a batched cell runs the recurrence on the first 64 queries of the
call only (a [N, 64] block per product), once per `steps`, and is stated per query.  Checked first against tests/diffuse_ref.py: every single
answer, and 8 columns of each batched call at steps = 3.  Reports per cell the new call, the route's own search, what the new
call adds to it, the baseline and its spread (max - min), the step kernels' microseconds and the bytes a step moves: the CSR
(12 B per stored edge, 8 B per row), the gathered f (8 C B per edge) and the written f (8 C B per row)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import diffuse_ref as dfr  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, make_queries, med  # noqa: E402

TAU, ALPHA = 0.62, 0.85
STEPS = (1, 3, 10)
L = asp._L
BASE = {}   # steps -> the batched baseline's per-query times

try:
    import scipy.sparse as sps
except ImportError:   # pragma: no cover
    sps = None


class HostOperator:
    """S on the host, prepared once: scipy's CSR, else segment sums with np.add.reduceat."""

    def __init__(self, op):
        self.ptr, self.col, self.S = op
        self.n = len(self.ptr) - 1
        self.how = "scipy.sparse" if sps is not None else "np.add.reduceat"
        if sps is not None:
            self.M = sps.csr_matrix((self.S, self.col, self.ptr), shape=(self.n, self.n))
        else:
            self.rows = np.flatnonzero(np.diff(self.ptr) > 0)

    def apply(self, f):
        if sps is not None:
            return self.M @ f
        prod = self.S * f[self.col] if f.ndim == 1 else self.S[:, None] * f[self.col]
        out = np.zeros_like(f)
        out[self.rows] = np.add.reduceat(prod, self.ptr[self.rows], axis=0)
        return out

    def diffuse(self, pools, steps, k):
        """The recurrence for a list of pools, then each query's first k by (f descending, index ascending)."""
        y = np.zeros((self.n, len(pools)))
        for b, pool in enumerate(pools):
            for i, v in pool:
                y[i, b] = v
        oy = (1.0 - ALPHA) * y
        f = y
        for _ in range(steps):
            f = ALPHA * self.apply(f) + oy
        out = []
        for b in range(len(pools)):
            col = f[:, b]
            top = np.argpartition(-col, k)[:k + 1]
            o = top[np.lexsort((top, -col[top]))][:k]
            out.append(list(zip(o.tolist(), col[o].tolist())))
        return out


def step_bytes(n, nnz, c):
    return nnz * 12 + (n + 1) * 8, nnz * 8 * c, n * 8 * c


def verdict(new, old):
    spread = max(old) - min(old)
    ok = med(new) < med(old) - spread
    return f"baseline spread {spread:.1f} us: " + ("the new call is below the baseline by more than it" if ok else
                                                   "the new call is NOT below the baseline by more than its spread")


def single_cell(aspace, gl, host, op, Q, steps, rounds, lines):
    n, nnz, k = host.n, len(op[1]), len(aspace.search(Q[0], gl, TAU))
    pools = [aspace.search(q, gl, TAU) for q in Q]
    Y = np.stack([dfr.seeds_vector(n, [i for i, _ in p], [v for _, v in p]) for p in pools], axis=1)
    F = dfr.diffuse(*op, Y, ALPHA, steps)
    same = 0
    for b, q in enumerate(Q):   # the answers, and the warm-up
        got = aspace.search_diffuse(q, gl, TAU, ALPHA, steps)
        want = dfr.rank(F[:, b], None, k)
        assert [i for i, _ in got] == [i for i, _ in want] and (dfr.canon([v for _, v in got]) == dfr.canon([v for _, v in want])).all()
        same += [i for i, _ in host.diffuse([pools[b]], steps, k)[0]] == [i for i, _ in got]
    t_s, t_new, t_old, ks = [], [], [], []
    for _ in range(rounds):
        for q in Q:
            t0 = time.perf_counter()
            aspace.search(q, gl, TAU)
            t1 = time.perf_counter()
            aspace.search_diffuse(q, gl, TAU, ALPHA, steps)
            t2 = time.perf_counter()
            host.diffuse([aspace.search(q, gl, TAU)], steps, k)
            t3 = time.perf_counter()
            t_s.append((t1 - t0) * 1e6)
            t_new.append((t2 - t1) * 1e6)
            t_old.append((t3 - t2) * 1e6)
    assert L.as_set_tuning(b"diffuse_timing", 1) == 0
    try:
        for q in Q:
            aspace.search_diffuse(q, gl, TAU, ALPHA, steps)
            ks.append(L.as_diffuse_kernel_us(aspace._h))
    finally:
        assert L.as_set_tuning(b"diffuse_timing", 0) == 0
    csr, gath, wr = step_bytes(n, nnz, 1)
    per_step = med(ks) / steps
    lines.append(f"steps={steps} B=1: search {med(t_s):.1f} us | search_diffuse {med(t_new):.1f} us (adds {med(np.array(t_new) - np.array(t_s)):.1f} us "
                 f"to search) | baseline (search + {host.how} on the host) {med(t_old):.1f} us | ratio {med(t_old) / med(t_new):.1f}x | {verdict(t_new, t_old)} | "
                 f"step kernels median {med(ks):.1f} us = {per_step:.1f} us per step; a step streams {csr / 1e6:.0f} MB of CSR = {csr / per_step / 1e6:.2f} TB/s "
                 f"of 8 TB/s, gathers {gath / 1e6:.0f} MB of f and writes {wr / 1e6:.0f} MB ({(csr + gath + wr) / per_step / 1e6:.2f} TB/s with both) | "
                 f"{len(Q)} answers equal diffuse_ref in bits, {same} baseline lists hold the same items")
    print(lines[-1], flush=True)


def batch_cell(aspace, gl, host, op, Qb, steps, rounds, mib, lines, check):
    n, nnz, b = host.n, len(op[1]), Qb.shape[0]
    assert L.as_set_tuning(b"diffuse_mib", mib) == 0
    try:
        pools = aspace.search_batch(Qb, gl, TAU)
        k = len(pools[0])
        got = aspace.search_batch_diffuse(Qb, gl, TAU, ALPHA, steps)
        if check:
            cols = list(range(0, b, max(b // 8, 1)))[:8]
            Y = np.stack([dfr.seeds_vector(n, [i for i, _ in pools[c]], [v for _, v in pools[c]]) for c in cols], axis=1)
            F = dfr.diffuse(*op, Y, ALPHA, steps)
            for j, c in enumerate(cols):
                want = dfr.rank(F[:, j], None, k)
                assert [i for i, _ in got[c]] == [i for i, _ in want] and (dfr.canon([v for _, v in got[c]]) == dfr.canon([v for _, v in want])).all()
        hb = min(b, 64)
        t_s, t_new, t_old = [], [], []
        for _ in range(rounds):
            t0 = time.perf_counter()
            aspace.search_batch(Qb, gl, TAU)
            t1 = time.perf_counter()
            aspace.search_batch_diffuse(Qb, gl, TAU, ALPHA, steps)
            t2 = time.perf_counter()
            t_s.append((t1 - t0) * 1e6 / b)
            t_new.append((t2 - t1) * 1e6 / b)
        if steps not in BASE:   # (seconds per call: two rounds, measured once per `steps` -- the same 64 queries in every batched cell)
            BASE[steps] = []
            for _ in range(2):
                t2 = time.perf_counter()
                host.diffuse(aspace.search_batch(np.ascontiguousarray(Qb[:hb]), gl, TAU), steps, k)
                BASE[steps].append((time.perf_counter() - t2) * 1e6 / hb)
        t_old = BASE[steps]
        assert L.as_set_tuning(b"diffuse_timing", 1) == 0
        try:
            c0 = aspace.diffuse_counters()
            aspace.search_batch_diffuse(Qb, gl, TAU, ALPHA, steps)
            ku = L.as_diffuse_kernel_us(aspace._h)
            chunks = aspace.diffuse_counters()["column chunks"] - c0["column chunks"]
        finally:
            assert L.as_set_tuning(b"diffuse_timing", 0) == 0
    finally:
        assert L.as_set_tuning(b"diffuse_mib", 0) == 0
    c = 64 if chunks * 16 < b else 16
    csr, gath, wr = step_bytes(n, nnz, c)
    per_step = ku / (steps * chunks)
    lines.append(f"steps={steps} B={b} diffuse_mib={mib} ({chunks} chunk(s) of {c} columns), per query: search_batch {med(t_s):.1f} us | "
                 f"search_batch_diffuse {med(t_new):.1f} us (adds {med(np.array(t_new) - np.array(t_s)):.1f} us) | baseline (search_batch + {host.how} "
                 f"over {hb} columns, 2 rounds) {med(t_old):.1f} us | ratio {med(t_old) / med(t_new):.1f}x | {verdict(t_new, t_old)} | step kernels "
                 f"{ku:.0f} us for the call = {ku / b / steps:.2f} us per query-step, {per_step:.1f} us per chunk-step: {csr / 1e6:.0f} MB of CSR, "
                 f"{gath / 1e6:.0f} MB of f gathered (re-reads, cache-served where they fit), {wr / 1e6:.0f} MB written = "
                 f"{(csr + gath + wr) / per_step / 1e6:.2f} TB/s with all three" + ("; 8 columns equal diffuse_ref in bits" if check else ""))
    print(lines[-1], flush=True)
    return med(t_new)


def main():
    argv = sys.argv[1:]
    n_items = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    nq = int(argv[2]) if len(argv) > 2 else 8
    rounds = int(argv[3]) if len(argv) > 3 else 5
    out = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "r21_diffuse.txt")
    X = gpu_clustered(n_items, d, 42)
    eps = calibrate_eps(X, 25)
    Q = make_queries(X, 1024, 43)
    gp = {"eps": eps, "k": 25, "topk": 100, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n_items, d, d)
    torch.cuda.synchronize()
    op = dfr.operator(*gl.to_csr())
    host = HostOperator(op)
    deg = np.diff(op[0])
    lines = [f"search_diffuse / search_batch_diffuse vs search + the recurrence on the host ({host.how}): N={n_items} D={d} k=25 topk=100 l2/gaussian "
             f"eps={eps:.5f} tau={TAU} alpha={ALPHA}; {len(op[1])} stored edges, longest row {int(deg.max())}, {int((deg == 0).sum())} rows without an edge; "
             f"{nq} queries x {rounds} rounds alternating; kernels = the step and seed kernels by HIP events (separate pass)"]
    print(lines[0], flush=True)
    for steps in STEPS:
        single_cell(aspace, gl, host, op, Q[:nq], steps, rounds, lines)
    best = {}
    for b in (64, 1024):
        Qb = np.ascontiguousarray(Q[:b])
        for steps in STEPS:
            for mib in (256, 1100):
                best[(b, steps, mib)] = batch_cell(aspace, gl, host, op, Qb, steps, rounds if b == 64 else max(rounds // 2, 2), mib, lines,
                                                   steps == 3 and b == 64)
    for (b, steps, mib), t in best.items():
        if mib == 256:
            t64 = best[(b, steps, 1100)]
            lines.append(f"B={b} steps={steps}: 16 columns per chunk {t:.1f} us per query, 64 columns per chunk {t64:.1f} us: "
                         f"{'16' if t <= t64 else '64'} columns are faster")
    lines.append(f"diffuse_counters {aspace.diffuse_counters()}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
