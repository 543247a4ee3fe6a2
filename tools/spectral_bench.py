"""Graph eigenpairs at the headline size: `ArrowSpace.eigsh` for m = 8 and 32 at tol = 1e-6 and 1e-8
against the route there was before -- scipy.sparse.linalg.eigsh(which="LA") and scipy.sparse.linalg.lobpcg with a block of C
columns over `to_csr()`'s matrix, prepared once outside the timing -- the routes alternating in one process.
python tools/spectral_bench.py [N] [D] [ROUNDS] [OUT] [BUDGET_S] [CELLS]  (defaults 1M x 768, 3 rounds,
profiles/r23_spectral.txt, 900 s for the host baselines, cells "8:1e-6,8:1e-8,32:1e-6,32:1e-8").

Data and index: tools/diffuse_bench.py's (clustered Gaussians, k = 25, topk = 100).  Every answer is checked first: the residuals
|S v - theta v| recomputed on the host (equal to the device's; <= 2 tol where the call converged) and orthonormality are
asserted; the values are compared with each baseline's position by position and the report says whether they agree within tol
(a single-vector Krylov method may miss copies of a multiple eigenvalue).  A call of either side that stops at its cap is
reported as not converged.  A baseline call runs under a cap on its work (about 1 500 products with S for scipy's eigsh, 60 / 20
iterations for lobpcg at 16 / 64 columns: a capped time is a lower bound); once the baselines have used BUDGET_S seconds, the
remaining baseline calls are left out and the report says so.  Criterion, the project's own: the new call's median is
below the baseline's by more than the baseline's own spread.  Then, by HIP events ("diffuse_timing", a separate pass): the time
per step, Gram, rotate and colnorm2 launch against the 2.7 ms recurrence step at C = 64 of section 5.22, and the shares of the
host's waits and of the host eigensolver in the call."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import scipy.sparse as sps  # noqa: E402
import scipy.sparse.linalg as spl  # noqa: E402
import torch  # noqa: E402

import diffuse_ref as dfr  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from range_bench import calibrate_eps, gpu_clustered, med  # noqa: E402

MAX_ITERS, DEGREE = 200, 16
EIGSH_MATVECS = 1500               # the cap on a scipy eigsh call: about this many products with S
LOBPCG_ITERS = {16: 60, 64: 20}    # the cap on a scipy lobpcg call, by block width
L = asp._L


def verdict(new, old):
    if len(old) < 2:
        return "fewer than two baseline runs: no spread, no verdict"
    spread = max(old) - min(old)
    ok = med(new) < med(old) - spread
    return f"baseline spread {spread / 1e3:.1f} ms: " + ("the new call is below the baseline by more than it" if ok else
                                                         "the new call is NOT below the baseline by more than its spread")


def agreement(w, values, tol):
    """A baseline's values against the new call's, position by position (a single-vector Krylov method may miss copies of a multiple
    eigenvalue: that shows here as a difference, and it is the baseline's)."""
    diff = float(np.abs(w - values).max())
    return f", its values {'agree with' if diff <= tol + 1e-12 else 'DIFFER from'} the new call's within tol (largest difference {diff:.1e}; its smallest {w[-1]:.12f})"


class Host:
    def __init__(self, op, budget):
        self.n = len(op[0]) - 1
        self.S = sps.csr_matrix((op[2], op[1], op[0]), shape=(self.n, self.n))
        self.budget, self.used = budget, 0.0

    def residuals(self, values, vectors):
        V = vectors.T
        return np.linalg.norm(self.S @ V - V * values[None, :], axis=0)

    def open(self):
        return self.used < self.budget

    def eigsh(self, m, tol):
        """-> (values descending or None, seconds, note)"""
        ncv = max(2 * m + 1, 20)
        restarts = max(10, EIGSH_MATVECS // (ncv - m))   # (a restart costs ncv - m products with S)
        t0 = time.perf_counter()
        try:
            w = spl.eigsh(self.S, k=m, ncv=ncv, which="LA", tol=tol, maxiter=restarts, return_eigenvectors=True)[0]
            note = "converged"
        except spl.ArpackNoConvergence as e:
            w, note = e.eigenvalues, f"NOT converged within {restarts} restarts ({len(e.eigenvalues)} of {m} values): the time is a lower bound"
        dt = time.perf_counter() - t0
        self.used += dt
        return (np.sort(w)[::-1] if len(w) == m else None), dt, note

    def lobpcg(self, m, C, tol, seed):
        X0 = np.random.default_rng(seed).standard_normal((self.n, C))
        t0 = time.perf_counter()
        w, _, hist = spl.lobpcg(self.S, X0, largest=True, tol=tol, maxiter=LOBPCG_ITERS[C], retResidualNormsHistory=True)
        dt = time.perf_counter() - t0
        self.used += dt
        res = np.asarray(hist[-1])
        note = f"{len(hist) - 1} iterations, " + ("converged" if (np.sort(res)[:m] <= tol).all() else f"NOT converged within its cap (the {m} best residuals up to {np.sort(res)[m - 1]:.1e}): the time is a lower bound")
        return np.sort(w)[::-1][:m], dt, note


def cell(aspace, gl, host, m, tol, rounds, lines):
    C = 16 if m <= 12 else 64
    c0 = aspace.eigsh_counters()
    values, vectors, info = aspace.eigsh(gl, m, tol, MAX_ITERS, DEGREE, with_info=True)   # the answer, and the warm-up
    c1 = aspace.eigsh_counters()
    true = host.residuals(values, vectors)
    defect = float(np.abs(vectors @ vectors.T - np.eye(m)).max())
    conv = info["converged"]   # (a call that stops at max_iters is reported as such: its values are not compared)
    assert defect <= 1e-10 and (not conv or (true <= 2.0 * tol).all()), (true.max(), defect)
    assert np.allclose(true, info["residuals"], rtol=1e-3, atol=1e-14), (true, info["residuals"])
    mult = int((values > 1.0 - max(tol, 1e-8)).sum())
    t_new, t_eig, t_lob, notes = [], [], [], {}
    for r in range(rounds):
        t0 = time.perf_counter()
        aspace.eigsh(gl, m, tol, MAX_ITERS, DEGREE)
        t_new.append((time.perf_counter() - t0) * 1e6)
        if host.open():
            w, dt, notes["eigsh"] = host.eigsh(m, tol)
            t_eig.append(dt * 1e6)
            if w is not None:
                notes["eigsh"] += agreement(w, values, tol)
        if host.open():
            w, dt, notes["lobpcg"] = host.lobpcg(m, C, tol, 100 + r)
            t_lob.append(dt * 1e6)
            notes["lobpcg"] += agreement(w, values, tol)
    d = {k: c1[k] - c0[k] for k in c1}
    line = (f"m={m} C={C} tol={tol}: eigsh {med(t_new) / 1e3:.1f} ms ({'converged' if conv else 'NOT converged at max_iters'}, {info['iterations']} outer iterations, {info['filter_steps']} steps, "
            f"{d['gram launches']} Grams, {d['rotate launches']} rotates, {d['host waits']} host waits; device residual up to {info['residuals'].max():.2e}, "
            f"host-recomputed up to {true.max():.2e}; orthonormality defect {defect:.1e}; {mult} of the {m} values are 1 within {max(tol, 1e-8):g}, "
            f"smallest returned {values[-1]:.12f})")
    for name, t in (("scipy eigsh(which='LA')", t_eig), (f"scipy lobpcg (block {C})", t_lob)):
        key = "eigsh" if "eigsh" in name else "lobpcg"
        if t:
            line += f" | {name} {med(t) / 1e3:.1f} ms over {len(t)} run(s), {notes[key]}: ratio {med(t) / med(t_new):.1f}x, {verdict(t_new, t)}"
        else:
            line += f" | {name}: left out (the baselines' budget of {host.budget:.0f} s was used up)"
    lines.append(line)
    print(line, flush=True)


def events_cell(aspace, gl, m, tol, lines):
    C = 16 if m <= 12 else 64
    assert L.as_set_tuning(b"diffuse_timing", 1) == 0
    try:
        c0 = aspace.eigsh_counters()
        _, _, info = aspace.eigsh(gl, m, tol, MAX_ITERS, DEGREE, with_info=True)
        c1 = aspace.eigsh_counters()
        us = [L.as_graph_eigs_kernel_us(aspace._h, p) for p in range(7)]
    finally:
        assert L.as_set_tuning(b"diffuse_timing", 0) == 0
    d = {k: c1[k] - c0[k] for k in c1}
    it = info["iterations"]
    per = (us[1] / d["step launches"], us[2] / d["gram launches"], us[3] / d["rotate launches"], us[4] / it)
    dev = sum(us[1:5])
    lines.append(f"m={m} C={C} tol={tol} by HIP events (every launch timed on its own, so the call is slower than untimed): call {us[0] / 1e3:.1f} ms; "
                 f"step {per[0]:.1f} us x {d['step launches']}, Gram with its tree {per[1]:.1f} us x {d['gram launches']}, rotate {per[2]:.1f} us x "
                 f"{d['rotate launches']}, colnorm2 with its tree {per[3]:.1f} us x {it}; of the device time {dev / 1e3:.1f} ms the steps are "
                 f"{100 * us[1] / dev:.0f}%, Grams {100 * us[2] / dev:.0f}%, rotates {100 * us[3] / dev:.0f}%, colnorm2 {100 * us[4] / dev:.0f}%; per outer iteration "
                 f"Gram + rotate are {100 * (us[2] + us[3]) / dev:.0f}% of the device time"
                 + (" -- MORE than the few percent expected" if (us[2] + us[3]) / dev > 0.1 else "") +
                 f"; host eigensolver {us[5] / 1e3:.1f} ms ({100 * us[5] / us[0]:.0f}% of the call), host waits {us[6] / 1e3:.1f} ms"
                 + (f"; a step against the 2.7 ms recurrence step of section 5.22: {per[0] / 2727.8:.2f}x" if C == 64 else ""))
    print(lines[-1], flush=True)


def main():
    argv = sys.argv[1:]
    n_items = int(argv[0]) if len(argv) > 0 else 1_000_000
    d = int(argv[1]) if len(argv) > 1 else 768
    rounds = int(argv[2]) if len(argv) > 2 else 3
    out = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "r23_spectral.txt")
    budget = float(argv[4]) if len(argv) > 4 else 900.0
    cells = [(int(a), float(b)) for a, b in (c.split(":") for c in (argv[5] if len(argv) > 5 else "8:1e-6,8:1e-8,32:1e-6,32:1e-8").split(","))]
    X = gpu_clustered(n_items, d, 42)
    eps = calibrate_eps(X, 25)
    gp = {"eps": eps, "k": 25, "topk": 100, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n_items, d, d)
    torch.cuda.synchronize()
    op = dfr.operator(*gl.to_csr())
    host = Host(op, budget)
    deg = np.diff(op[0])
    lines = [f"eigsh vs scipy.sparse.linalg.eigsh(which='LA') and lobpcg on the host over to_csr()'s matrix: N={n_items} D={d} k=25 topk=100 l2/gaussian "
             f"eps={eps:.5f}; {len(op[1])} stored edges, longest row {int(deg.max())}, {int((deg == 0).sum())} rows without an edge; max_iters={MAX_ITERS} "
             f"degree={DEGREE}; {rounds} rounds alternating; the host baselines share a budget of {budget:.0f} s"]
    print(lines[0], flush=True)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

    for m, tol in cells:
        cell(aspace, gl, host, m, tol, rounds, lines)
        flush()
    for m, tol in cells:
        events_cell(aspace, gl, m, tol, lines)
        flush()
    lines.append(f"eigsh_counters {aspace.eigsh_counters()}")
    flush()


if __name__ == "__main__":
    main()
