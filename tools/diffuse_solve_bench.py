"""Fixed-point diffusion search at the headline size: `search_diffuse_solve` (B = 1) and
`search_batch_diffuse_solve` (B = 1024, under "diffuse_cols" = 16 and 64) at alpha = 0.85 and 0.99, tol = 1e-6, against
(i) the route there was before for this answer -- `search` (`search_batch`), then conjugate gradients on the host over
`to_csr()`'s matrix (scipy.sparse's CSR and scipy.sparse.linalg.cg if importable, else tests/diffuse_solve_ref.py), prepared once
outside the timing -- and (ii) `search_diffuse` (`search_batch_diffuse`) at steps = 64, its cap, the three alternating in one
process; the relative residual |b - (I - alpha S) f| / |b| each of the three reaches stands beside the times.
python tools/diffuse_solve_bench.py [N] [D] [NQ] [ROUNDS] [OUT] [B]  (defaults 1M x 768, 8 queries, 5 rounds,
profiles/r22_diffuse_solve.txt, B = 1024).

Data and index: tools/diffuse_bench.py's (clustered Gaussians, k = 25, topk = 100, tau = 0.62).  Checked first against
tests/diffuse_solve_ref.py on `to_csr()`: every single answer (list, score bits, iterations, residual), and the first 8 queries
of every batched call (whose pools are the single route's where the two routes return the same lists).  Medians over queries x
rounds (B = 1) or over rounds, per query (batched; the host baseline of a batched cell solves the first 16 queries of the call,
two rounds).  Then, by HIP events (as_set_tuning("diffuse_timing"), a separate pass, C = 1 / 16 / 64 columns): one iteration --
the span of the loop divided by the iterations launched, host waits included -- against one step of the recurrence, and the five
launches of a sampled iteration (as_diffuse_solve_kernel_us parts 1 .. 5); what the span holds beyond the five is the host's
wait and launch gaps.  Bytes of an iteration: the CSR (12 B per stored edge, 8 B per row), p gathered (8 C B per edge), and 8 C B
per row for each vector pass: apply reads p and writes q (2), update reads x, p, r, q and writes x, r (6), direction reads r, p
and writes p (3)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import diffuse_ref as dfr  # noqa: E402
import diffuse_solve_ref as dsr  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, make_queries, med  # noqa: E402

TAU, TOL, MAX_ITERS = 0.62, 1e-6, 100
ALPHAS = (0.85, 0.99)
L = asp._L

try:
    import scipy.sparse as sps
    import scipy.sparse.linalg as spl
except ImportError:   # pragma: no cover
    sps = spl = None


class HostSolver:
    """(I - alpha S) on the host, prepared once per alpha: scipy's CSR and cg, else the numpy reference."""

    def __init__(self, op):
        self.op = op
        self.n = len(op[0]) - 1
        self.how = "scipy.sparse.linalg.cg" if sps is not None else "tests/diffuse_solve_ref.py"
        self.S = sps.csr_matrix((op[2], op[1], op[0]), shape=(self.n, self.n)) if sps is not None else None
        self.A = {}

    def matrix(self, alpha):
        if alpha not in self.A:
            self.A[alpha] = (sps.identity(self.n, format="csr") - alpha * self.S).tocsr()
        return self.A[alpha]

    def residual(self, alpha, y, f):
        b = (1.0 - alpha) * y
        r = b - self.matrix(alpha) @ f if sps is not None else b - (f - alpha * dsr.RowSums(*self.op)(f))
        return float(np.linalg.norm(r) / np.linalg.norm(b))

    def solve(self, pools, alpha, k):
        """CG per pool to TOL, then each query's first k by (f descending, index ascending)."""
        out = []
        for pool in pools:
            y = np.zeros(self.n)
            for i, v in pool:
                y[i] = v
            if sps is not None:
                try:
                    f, _ = spl.cg(self.matrix(alpha), (1.0 - alpha) * y, rtol=TOL, atol=0.0, maxiter=MAX_ITERS)
                except TypeError:   # (scipy before 1.12 calls it tol)
                    f, _ = spl.cg(self.matrix(alpha), (1.0 - alpha) * y, tol=TOL, atol=0.0, maxiter=MAX_ITERS)
            else:
                f = dsr.solve(*self.op, y, alpha, TOL, MAX_ITERS)[0]
            top = np.argpartition(-f, k)[:k + 1]
            o = top[np.lexsort((top, -f[top]))][:k]
            out.append(list(zip(o.tolist(), f[o].tolist())))
        return out


def pool_vector(n, pool):
    return dfr.seeds_vector(n, [i for i, _ in pool], [v for _, v in pool])


def pool_seeds(pool):
    return (np.array([i for i, _ in pool], dtype=np.int64), np.array([v for _, v in pool], dtype=np.float64))


def same_list(got, want):
    return [i for i, _ in got] == [i for i, _ in want] and (dfr.canon([v for _, v in got]) == dfr.canon([v for _, v in want])).all()


def verdict(new, old):
    spread = max(old) - min(old)
    ok = med(new) < med(old) - spread
    return f"baseline spread {spread:.1f} us: " + ("the new call is below the baseline by more than it" if ok else
                                                   "the new call is NOT below the baseline by more than its spread")


def iteration_bytes(n, nnz, c):
    return nnz * 12 + (n + 1) * 8, nnz * 8 * c, 11 * n * 8 * c


class Refs:
    """The numpy reference of a pool at an alpha, computed once (keyed by the pool itself)."""

    def __init__(self, op):
        self.op, self.n, self.memo = op, len(op[0]) - 1, {}

    def get(self, pools, alpha):
        todo = [p for p in pools if (alpha, tuple(p)) not in self.memo]
        if todo:
            Y = np.stack([pool_vector(self.n, p) for p in todo], axis=1)
            F, it, res, conv = dsr.solve(*self.op, Y, alpha, TOL, MAX_ITERS)
            for j, p in enumerate(todo):
                self.memo[(alpha, tuple(p))] = (F[:, j].copy(), int(it[j]), float(res[j]), bool(conv[j]))
        return [self.memo[(alpha, tuple(p))] for p in pools]


def single_cell(aspace, gl, host, refs, Q, alpha, rounds, lines):
    n = host.n
    pools = [aspace.search(q, gl, TAU) for q in Q]
    k = len(pools[0])
    want = refs.get(pools, alpha)
    its, res_new, res_true, res_64, res_host, same = [], [], [], [], [], 0
    for b, q in enumerate(Q):   # the answers, and the warm-up
        got, info = aspace.search_diffuse_solve(q, gl, TAU, alpha, TOL, MAX_ITERS, with_info=True)
        f, it, res, conv = want[b]
        assert same_list(got, dfr.rank(f, None, k)) and (info["iterations"], info["residual"], info["converged"]) == (it, res, conv), (b, info, it, res)
        y = pool_vector(n, pools[b])
        raw, _ = aspace.diffuse_solve(gl, [pool_seeds(pools[b])], alpha, TOL, MAX_ITERS)
        res_true.append(host.residual(alpha, y, raw[0]))
        res_64.append(host.residual(alpha, y, aspace.diffuse(gl, [pool_seeds(pools[b])], alpha, 64)[0]))
        base = host.solve([pools[b]], alpha, k)[0]
        same += [i for i, _ in base] == [i for i, _ in got]
        its.append(it)
        res_new.append(res)
    t_s, t_new, t_old, t_64 = [], [], [], []
    for _ in range(rounds):
        for q in Q:
            t0 = time.perf_counter()
            aspace.search(q, gl, TAU)
            t1 = time.perf_counter()
            aspace.search_diffuse_solve(q, gl, TAU, alpha, TOL, MAX_ITERS)
            t2 = time.perf_counter()
            host.solve([aspace.search(q, gl, TAU)], alpha, k)
            t3 = time.perf_counter()
            aspace.search_diffuse(q, gl, TAU, alpha, 64)
            t4 = time.perf_counter()
            t_s.append((t1 - t0) * 1e6)
            t_new.append((t2 - t1) * 1e6)
            t_old.append((t3 - t2) * 1e6)
            t_64.append((t4 - t3) * 1e6)
    lines.append(f"alpha={alpha} tol={TOL} B=1: search {med(t_s):.1f} us | search_diffuse_solve {med(t_new):.1f} us ({min(its)}-{max(its)} iterations, "
                 f"reported residual up to {max(res_new):.2e}, true residual up to {max(res_true):.2e}) | baseline (search + {host.how} on the host) "
                 f"{med(t_old):.1f} us | ratio {med(t_old) / med(t_new):.1f}x | {verdict(t_new, t_old)} | search_diffuse at steps=64 {med(t_64):.1f} us, "
                 f"true residual {min(res_64):.2e}-{max(res_64):.2e} ({med(t_64) / med(t_new):.2f}x the solve's time) | {len(Q)} answers, iteration counts "
                 f"and residuals equal diffuse_solve_ref in bits, {same} baseline lists hold the same items")
    print(lines[-1], flush=True)


def batch_cell(aspace, gl, host, refs, Qb, alpha, rounds, cols, lines, base):
    b = Qb.shape[0]
    assert L.as_set_tuning(b"diffuse_cols", cols) == 0
    try:
        pools = aspace.search_batch(Qb, gl, TAU)
        k = len(pools[0])
        c0 = aspace.diffuse_solve_counters()
        got, info = aspace.search_batch_diffuse_solve(Qb, gl, TAU, alpha, TOL, MAX_ITERS, with_info=True)
        c1 = aspace.diffuse_solve_counters()
        want = refs.get(pools[:8], alpha)
        for j in range(8):
            f, it, res, conv = want[j]
            assert same_list(got[j], dfr.rank(f, None, k)), j
            assert (int(info["iterations"][j]), float(info["residual"][j]), bool(info["converged"][j])) == (it, res, conv), j
        assert info["converged"].all()
        aspace.search_batch_diffuse(Qb, gl, TAU, alpha, 64)   # (warm-up)
        t_s, t_new, t_64 = [], [], []
        for _ in range(rounds):
            t0 = time.perf_counter()
            aspace.search_batch(Qb, gl, TAU)
            t1 = time.perf_counter()
            aspace.search_batch_diffuse_solve(Qb, gl, TAU, alpha, TOL, MAX_ITERS)
            t2 = time.perf_counter()
            aspace.search_batch_diffuse(Qb, gl, TAU, alpha, 64)
            t3 = time.perf_counter()
            t_s.append((t1 - t0) * 1e6 / b)
            t_new.append((t2 - t1) * 1e6 / b)
            t_64.append((t3 - t2) * 1e6 / b)
        hb = min(b, 16)
        if alpha not in base:   # (two rounds, once per alpha: the same 16 queries in every batched cell)
            base[alpha] = []
            for _ in range(2):
                t2 = time.perf_counter()
                host.solve(aspace.search_batch(np.ascontiguousarray(Qb[:hb]), gl, TAU), alpha, k)
                base[alpha].append((time.perf_counter() - t2) * 1e6 / hb)
        t_old = base[alpha]
    finally:
        assert L.as_set_tuning(b"diffuse_cols", 0) == 0
    chunks = c1["column chunks"] - c0["column chunks"]
    launched = c1["iterations launched"] - c0["iterations launched"]
    it = info["iterations"]
    lines.append(f"alpha={alpha} tol={TOL} B={b} diffuse_cols={cols} ({chunks} chunk(s)), per query: search_batch {med(t_s):.1f} us | "
                 f"search_batch_diffuse_solve {med(t_new):.1f} us (iterations {int(it.min())}-{int(it.max())}, mean {it.mean():.1f}; {launched} chunk-iterations "
                 f"launched = {launched * cols / b:.1f} per query slot; residual up to {info['residual'].max():.2e}) | baseline (search_batch + {host.how} "
                 f"over {hb} queries, 2 rounds) {med(t_old):.1f} us | ratio {med(t_old) / med(t_new):.1f}x | {verdict(t_new, t_old)} | "
                 f"search_batch_diffuse at steps=64 {med(t_64):.1f} us ({med(t_64) / med(t_new):.2f}x the solve's time) | 8 queries equal diffuse_solve_ref in bits")
    print(lines[-1], flush=True)


def events_cell(aspace, gl, host, Q, alpha, cols, lines):
    """One iteration against one step by HIP events, and the five launches of a sampled iteration."""
    n, nnz = host.n, len(host.op[1])
    nb = {1: 1, 16: 16, 64: 64}[cols]
    Qb = np.ascontiguousarray(Q[:nb])
    assert L.as_set_tuning(b"diffuse_cols", cols) == 0 and L.as_set_tuning(b"diffuse_timing", 1) == 0
    try:
        spans, parts, steps_us, iters = [], [], [], []
        for _ in range(3):
            c0 = aspace.diffuse_solve_counters()
            aspace.search_batch_diffuse_solve(Qb, gl, TAU, alpha, TOL, MAX_ITERS)
            c1 = aspace.diffuse_solve_counters()
            launched = c1["iterations launched"] - c0["iterations launched"]
            iters.append(launched)
            spans.append(L.as_diffuse_solve_kernel_us(aspace._h, 0) / launched)
            parts.append([L.as_diffuse_solve_kernel_us(aspace._h, p) for p in range(1, 6)])
            aspace.search_batch_diffuse(Qb, gl, TAU, alpha, 16)
            steps_us.append(L.as_diffuse_kernel_us(aspace._h) / 16)
    finally:
        assert L.as_set_tuning(b"diffuse_cols", 0) == 0 and L.as_set_tuning(b"diffuse_timing", 0) == 0
    span, step = med(spans), med(steps_us)
    pt = [med([p[j] for p in parts]) for j in range(5)]
    csr, gath, vec = iteration_bytes(n, nnz, cols)
    names = ("apply", "reduce p.q", "update", "reduce r.r", "direction + copy of the scalars")
    lines.append(f"alpha={alpha} C={cols}: one iteration {span:.1f} us (loop span / {iters[-1]} iterations, host waits included) against one recurrence "
                 f"step {step:.1f} us = {span / step:.2f}x | sampled iteration: " + ", ".join(f"{nm} {v:.1f} us" for nm, v in zip(names, pt)) +
                 f"; the five sum to {sum(pt):.1f} us ({100 * sum(pt) / span:.0f}% of an iteration; the four small launches {100 * (sum(pt) - pt[0]) / span:.0f}%, "
                 f"host wait and gaps {100 * max(span - sum(pt), 0.0) / span:.0f}%) | apply against a step {pt[0] / step:.2f}x | an iteration moves "
                 f"{csr / 1e6:.0f} MB of CSR, gathers {gath / 1e6:.0f} MB of p and streams {vec / 1e6:.0f} MB of vectors = "
                 f"{(csr + gath + vec) / span / 1e6:.2f} TB/s with all three; update alone {6 * n * 8 * cols / pt[2] / 1e6:.2f} TB/s, "
                 f"direction {3 * n * 8 * cols / pt[4] / 1e6:.2f} TB/s")
    print(lines[-1], flush=True)


def main():
    argv = sys.argv[1:]
    n_items = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    nq = int(argv[2]) if len(argv) > 2 else 8
    rounds = int(argv[3]) if len(argv) > 3 else 5
    out = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "r22_diffuse_solve.txt")
    bsz = int(argv[5]) if len(argv) > 5 else 1024
    X = gpu_clustered(n_items, d, 42)
    eps = calibrate_eps(X, 25)
    Q = make_queries(X, max(bsz, 64), 43)
    gp = {"eps": eps, "k": 25, "topk": 100, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n_items, d, d)
    torch.cuda.synchronize()
    op = dfr.operator(*gl.to_csr())
    host = HostSolver(op)
    refs = Refs(op)
    deg = np.diff(op[0])
    lines = [f"search_diffuse_solve / search_batch_diffuse_solve vs search + CG on the host ({host.how}) and vs search_diffuse at steps=64: N={n_items} D={d} "
             f"k=25 topk=100 l2/gaussian eps={eps:.5f} tau={TAU} tol={TOL} max_iters={MAX_ITERS}; {len(op[1])} stored edges, longest row {int(deg.max())}, "
             f"{int((deg == 0).sum())} rows without an edge; {nq} queries x {rounds} rounds alternating; residuals are |b - (I - alpha S) f| / |b| on the host"]
    print(lines[0], flush=True)
    for alpha in ALPHAS:
        single_cell(aspace, gl, host, refs, Q[:nq], alpha, rounds, lines)
    base = {}
    Qb = np.ascontiguousarray(Q[:bsz])
    for alpha in ALPHAS:
        for cols in (16, 64):
            batch_cell(aspace, gl, host, refs, Qb, alpha, max(rounds // 2, 2), cols, lines, base)
    for cols in (1, 16, 64):
        events_cell(aspace, gl, host, Q, 0.85, cols, lines)
    lines.append("the fused apply kernel against an unfused pair (step kernel + a dot pass): not measured, the unfused pair was never built")
    lines.append(f"diffuse_solve_counters {aspace.diffuse_solve_counters()}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
