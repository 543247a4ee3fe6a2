#!/usr/bin/env python3
"""bench.py -- queries/sec + index-build seconds on synthetic N x D fp32 (BASELINE.json).

    python bench.py --gpus 1 --steps K --warmup W            (default N=1M, D=768)
    python -m torch.distributed.run --nproc-per-node G ... bench.py --gpus G ...
    python bench.py --gpus G ...                             (no launcher: spawns its G ranks itself, see launch())

One "step" = one ArrowSpace.search() call (one query, full scan over the N items,
lambda_q + blended scorer + top-k) -- the reference's harnesses issue one query per call
(tests/test_4_msmarco_tau_sweep.py:216).  The index build runs once before the timed
region and is reported next to it (index_build_sec).  Inputs are resident in HBM when
either timed region starts.  Rank 0 prints ONE JSON line.

A plain run does what the headline needs: data, index build, W warmup + K timed searches, the line.  --full adds
every side measurement and check (roofline figures, in-distribution queries, threads, batched search, fp64
brute-force verification, unfriendly distributions, the build from host memory, CPU baseline).
--dump-outputs DIR writes the hits of the last timed search; the inputs depend on the arguments alone.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

# The library runs up to a dozen HIP streams of its own (a pool of single-query workspaces for concurrent callers, two pairs of
# batched workspaces); the ROCm runtime multiplexes a process's streams over 4 hardware queues unless told otherwise, and
# streams that share a queue run strictly one kernel after the other ("Hardware queues").  Read at the first
# HIP call: set before torch is imported.  (Same box, tools/hwq_bench_ab.sh: batched 98 000 -> 117 000-120 000 queries/s, B = 1 unchanged.)
# Only when this file is the program: a test or tool that imports it keeps the runtime's default.
if __name__ == "__main__":
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_F32_PEAK_TF = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
MFMA_F64_PEAK_TF = 78.6    # v_mfma_f64_16x16x4_f64: vendor fp64 matrix peak (half the fp32 rate; not in the guide's table)
MFMA_BF16_PEAK_TF = 2500.0 # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_bf16 dense peak (never the 2:1 sparsity figure)
MFMA_I8_PEAK_TOPS = 5000.0 # v_mfma_i32_32x32x32_i8 / _16x16x64_i8: the cycles of the bf16 form of the same M x N at twice the K (MI355X_MICROARCH.md, matrix cores table)


def launch(n_ranks, argv, child=None):
    """`python bench.py --gpus N` without a launcher around it: start N fresh processes, one per rank, BEFORE anything in
    this process has touched the GPU (this parent never does: it imports no torch, makes no HIP call), hand them the
    rendezvous through the environment torch.distributed.run would set, relay what they print and return the worst exit
    code.  Rank r takes device r; on a box with fewer devices than ranks (one-GPU rehearsal of an N-rank job) the ranks
    share the devices round-robin and the exchange steps are staged through host memory (ARROWSPACE_BENCH_SHARED_GPU,
    pyarrowspace_amd.dist.HostStagedIndex) -- RCCL wants one device per rank."""
    import socket
    import subprocess

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ndev = int(os.environ.get("ARROWSPACE_BENCH_NDEV", "0")) or visible_devices()
    shared = ndev < n_ranks
    cmd = list(child) if child is not None else [sys.executable, os.path.abspath(__file__)]
    import signal
    import time

    procs = []
    for r in range(n_ranks):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r % max(ndev, 1)), WORLD_SIZE=str(n_ranks), LOCAL_WORLD_SIZE=str(n_ranks),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        if shared:
            env["ARROWSPACE_BENCH_SHARED_GPU"] = str(max(ndev, 1))
        # a session (= process group) of its own per rank: what it started dies with it when the group is signalled
        procs.append(subprocess.Popen(cmd + list(argv), env=env, start_new_session=True))

    def code(rc):
        return rc if rc >= 0 else 128 - rc

    def stop_all(grace_s=10.0):
        """SIGTERM to every live rank's process group, SIGKILL to what is still there after the grace period."""
        for sig in (signal.SIGTERM, signal.SIGKILL):
            live = [p for p in procs if p.poll() is None]
            if not live:
                return
            for p in live:
                try:
                    os.killpg(p.pid, sig)
                except (ProcessLookupError, PermissionError):
                    pass
            t_end = time.monotonic() + grace_s
            while time.monotonic() < t_end and any(p.poll() is None for p in live):
                time.sleep(0.05)

    # All ranks are polled together: the first one that fails takes the others down (they would otherwise sit in a
    # rendezvous or a collective their peer never enters) and its code is the launch's; so does an interrupt or the
    # overall time limit (ARROWSPACE_BENCH_LAUNCH_TIMEOUT seconds, 0 = none).
    limit = float(os.environ.get("ARROWSPACE_BENCH_LAUNCH_TIMEOUT", "0") or 0)
    t0 = time.monotonic()
    worst = 0
    try:
        while True:
            rcs = [p.poll() for p in procs]
            failed = [code(rc) for rc in rcs if rc is not None and rc != 0]
            if failed:
                worst = max(failed)
                stop_all()
                break
            if all(rc is not None for rc in rcs):
                break
            if limit and time.monotonic() - t0 > limit:
                print("bench.launch: ranks still running after %.0f s: stopping them" % limit, file=sys.stderr, flush=True)
                stop_all()
                worst = 124
                break
            time.sleep(0.05)
    except KeyboardInterrupt:
        stop_all()
        worst = 130
    for p in procs:   # (every rank has exited or been killed: reap, and fold in codes that arrived meanwhile)
        rc = p.wait()
        if rc > 0:   # ranks this launcher signalled itself (negative codes) do not outrank the failure that caused it
            worst = max(worst, rc)
    return worst


def visible_devices():
    """GPUs this process may use, counted without initialising any: the KFD topology's nodes with SIMDs, cut down by
    HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES when set."""
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None and v.strip() != "":
            return len([x for x in v.split(",") if x.strip() != ""])
    n = 0
    base = "/sys/class/kfd/kfd/topology/nodes"
    try:
        for node in os.listdir(base):
            try:
                props = open(os.path.join(base, node, "properties")).read()
            except OSError:
                continue
            for line in props.splitlines():
                if line.startswith("simd_count") and int(line.split()[1]) > 0:
                    n += 1
    except OSError:
        pass
    return n


def live_traffic(workload_argv, timeout_s=150):
    """HBM-side bytes per launch of the roofline kernels, measured NOW rather than read from a committed profile: two
    child runs of this file (a short pass of the same workload: the build, 22 searches, the batched passes) under
    rocprofv3, one --pmc pass per counter (FETCH_SIZE, WRITE_SIZE) as MI355X_MICROARCH.md's HBM section prescribes,
    summarised and corrected by profiles/summarise.py (the x2 of 16-byte-per-lane streaming reads on gfx950).  Called
    before this process touches the GPU; the children have the card to themselves.  Returns (dict kernel -> bytes per
    launch, note) -- (None, why) when rocprofv3 is not on this box, is already around this process, or a pass fails."""
    import shutil
    import subprocess
    import tempfile

    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not found"
    if any(k.startswith("ROCPROF") for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
        return None, "already under a profiler"
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import summarise

    tmp = tempfile.mkdtemp(prefix="as_traffic_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        csvs = {}
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, counter)
            cmd = [exe, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", out, "--",
                   sys.executable, os.path.abspath(__file__), "--traffic-probe", "--full", "--no-cpu-baseline", "--steps", "20", "--warmup", "2"] + list(workload_argv)
            with open(os.path.join(tmp, counter + ".log"), "w") as log:
                # (its own process group: a pass that runs out of time is ended with everything it started -- the profiled
                # child must not keep the GPU busy under the measurement that follows)
                proc = subprocess.Popen(cmd, env=env, cwd=ROOT, stdout=log, stderr=subprocess.STDOUT, start_new_session=True)
                try:
                    rc = proc.wait(timeout=timeout_s)
                except subprocess.TimeoutExpired:
                    import signal
                    try:
                        os.killpg(proc.pid, signal.SIGKILL)
                    except OSError:
                        pass
                    proc.wait()
                    return None, "%s pass timed out after %d s" % (counter, timeout_s)
            if rc != 0:
                print("bench.py: live traffic pass (%s) failed:\n%s" % (counter, open(os.path.join(tmp, counter + ".log")).read()[-600:]), file=sys.stderr)
                return None, "%s pass exited with %d" % (counter, rc)
            csvs[counter] = os.path.join(tmp, counter + ".csv")
            with open(os.devnull, "w") as null:
                stdout, sys.stdout = sys.stdout, null
                try:
                    summarise.pmc(out, counter, csvs[counter])
                finally:
                    sys.stdout = stdout
        with open(os.devnull, "w") as null:
            stdout, sys.stdout = sys.stdout, null
            try:
                summarise.traffic(csvs["FETCH_SIZE"], csvs["WRITE_SIZE"], 0, 0, os.path.join(tmp, "traffic.json"))
            finally:
                sys.stdout = stdout
        doc = json.load(open(os.path.join(tmp, "traffic.json")))
        got = {k: v["bytes_per_launch"] for k, v in doc.items() if isinstance(v, dict) and "bytes_per_launch" in v}
        return (got, "live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload run by this bench.py (2 x FETCH_SIZE KiB + WRITE_SIZE KiB, "
                     "MI355X_MICROARCH.md HBM section)") if got else (None, "no kernel of the path in the counter output")
    except Exception as e:      # noqa: BLE001 -- a broken profiler must not cost the measurement
        return None, "%s: %s" % (type(e).__name__, e)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


PARITY = {
    "status": "partial",
    "pinned_by_reference": "scorer form only: README 3x3 scores to 1e-12 (README.md:69), tests/test_0.py tau=1.0 order (:28-32), "
                           "37 recorded (cos, lambda-term, tau=.62) triples of tests/output/1761047573_v0_17/cve_search_results.csv",
    "unpinned": "graph topology, Laplacian entries and every lambda: the arithmetic lives in crates.io arrowspace 0.18.0, not in the "
                "tree and not buildable here; results are rank-exact against this repo's own fp64 oracle of its SPEC (DESIGN.md 2-3)",
    "test_0_tau_lt_1_orders_met": "0/3 (tests/test_0.py:34-61; profiles/r03_test0_families.md: 58 752 lambda variants tried)",
}


def make_data(n, d, seed, device, nclust=1024, noise=0.5, return_centres=False):
    """SURVEY section 8(d) recipe, bit for bit and reproducible off the GPU: rng = np.random.default_rng(seed);
    C = rng.standard_normal((nclust, d)); z = rng.integers(0, nclust, n); X = C[z] + noise * rng.standard_normal((n, d));
    rows L2-normalised; cast fp32.  The noise is drawn in row chunks (the generator's stream is the same as for one
    big call) so the host holds a few fp64 chunks, never the whole array.  The draws are serial; the rest of a chunk (centres,
    normalisation, cast, copy) runs on a second thread under the next chunk's draw -- numpy and the copy release the
    interpreter lock -- which takes about a third off the recipe's host time at 1M x 768 and changes no bit."""
    from concurrent.futures import ThreadPoolExecutor

    import torch

    rng = np.random.default_rng(seed)
    C = rng.standard_normal((nclust, d))
    z = rng.integers(0, nclust, n)
    X = torch.empty((n, d), device=device, dtype=torch.float32)

    def finish(s, e, draw):
        blk = C[z[s:e]] + noise * draw
        blk /= np.linalg.norm(blk, axis=1, keepdims=True)
        X[s:e] = torch.from_numpy(blk.astype(np.float32)).to(device)

    step = 1 << 16
    with ThreadPoolExecutor(1) as pool:
        pending = None
        for s in range(0, n, step):
            e = min(n, s + step)
            draw = rng.standard_normal((e - s, d))
            if pending is not None:
                pending.result()
            pending = pool.submit(finish, s, e, draw)
        pending.result()
    return (X, C) if return_centres else X


def make_queries_in_distribution(C, nq, seed, noise=0.5):
    """SURVEY 8(d) queries: fresh draws of the recipe around the SAME centres -- cluster labels and noise from
    np.random.default_rng(seed), rows normalised.  (New centres would have no item within eps of any query.)"""
    rng = np.random.default_rng(seed)
    z = rng.integers(0, C.shape[0], nq)
    Q = C[z] + noise * rng.standard_normal((nq, C.shape[1]))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return Q


def make_queries(X, nq, seed, spread=0.02):
    """Queries: perturbed items, rows picked and noise drawn from np.random.default_rng(seed) -- as
    tests/test_0.py:24 queries with a scaled item -- so that every query has neighbours inside eps (a fresh
    sample of the section-8(d) recipe has its own cluster centres: no item within eps, lambda_q = 0, and the
    reference's assert, src/lib.rs:156-159, would end the run).  Recorded as a deviation in config.workload."""
    rng = np.random.default_rng(seed)
    n, d = X.shape
    rows = rng.integers(0, n, nq)
    Q = X[rows].double().cpu().numpy() + spread * rng.standard_normal((nq, d)) / np.sqrt(d)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return Q


def make_data_torch(kind, n, d, seed, device):
    """The unfriendly distributions of the sweep (bench side keys, tools/dist_sweep.py), drawn on the GPU from
    torch.Generator(seed), rows normalised, fp32:
      isotropic -- standard normal rows: every pairwise cosine ~ N(0, 1/d), no cluster to stand out of;
      hier      -- 1 024 centres around 16 super-centres on top of ONE common direction (squared-norm shares 0.45 common,
                   0.15 super-centre, 0.20 centre, 0.20 noise): background cosine 0.45-0.6 between unrelated rows, 0.8 inside a
                   cluster -- what sentence embeddings with a large common mean look like;
      scaled100 -- SURVEY 8(d)'s clustered recipe times 100, unnormalised (/root/reference/tests/test_3_beir.py:19,190)."""
    import torch

    g = torch.Generator(device=device)
    g.manual_seed(seed)
    X = torch.empty((n, d), device=device, dtype=torch.float32)

    def rn(*shape):
        return torch.randn(*shape, generator=g, device=device, dtype=torch.float32)

    if kind == "isotropic":
        parts = None
    elif kind == "hier":
        common = rn(1, d)
        sup = rn(16, d)
        cen = rn(1024, d)
        zs = torch.randint(0, 16, (1024,), generator=g, device=device)
        parts = (0.45 ** 0.5) * common + (0.15 ** 0.5) * sup[zs] + (0.20 ** 0.5) * cen     # [1024, d]
    elif kind == "scaled100":
        parts = rn(1024, d)
    else:
        raise ValueError(kind)
    step = 1 << 17
    for s in range(0, n, step):
        e = min(n, s + step)
        if kind == "isotropic":
            blk = rn(e - s, d)
        else:
            z = torch.randint(0, 1024, (e - s,), generator=g, device=device)
            blk = parts[z] + (0.20 ** 0.5 if kind == "hier" else 0.5) * rn(e - s, d)
        blk /= blk.norm(dim=1, keepdim=True)
        X[s:e] = blk * (100.0 if kind == "scaled100" else 1.0)
    return X


def brute_force_verify(aspace, gl, X, queries, tau, topk, rtol=1e-9, want=None):
    """The library's hits for `queries` against an fp64 brute force on the GPU (torch): cosines of ALL items in fp64,
    TAUMODE.md:33's score with the library's own lambda_q and lambdas, top-k by (score desc, index asc).  A query counts
    as a mismatch when its scores differ beyond rtol or its indices differ anywhere outside a run of scores equal to
    1e-12.  Queries whose lambda_q is zero (the reference's panic, src/lib.rs:156-159) are skipped and counted.
    Returns {"n", "mismatches", "zero_lambda"}."""
    import torch

    import pyarrowspace_amd as asp

    dev = X.device
    got, lqs, keep = [], [], []
    zero = 0
    for q in queries:
        q = np.ascontiguousarray(q, dtype=np.float64)
        try:
            hits = aspace.search(q, gl, tau)
        except asp.PanicException:
            zero += 1
            continue
        got.append(hits)
        lqs.append(aspace.query_lambda(q, gl))
        keep.append(q)
        if want is not None and len(keep) >= want:   # (the first `want` queries that have an answer: the rest of `queries` are spares)
            break
    if not keep:
        return {"n": 0, "mismatches": 0, "zero_lambda": zero}
    Qd = torch.from_numpy(np.stack(keep)).to(dev)                       # [nq, d] fp64
    qn = (Qd * Qd).sum(1).sqrt()
    lam = torch.from_numpy(aspace.lambdas()).to(dev)
    lq = torch.tensor(lqs, dtype=torch.float64, device=dev)
    n = X.shape[0]
    best_s = torch.full((len(keep), 0), 0.0, dtype=torch.float64, device=dev)
    best_i = torch.zeros((len(keep), 0), dtype=torch.int64, device=dev)
    kk = min(topk + 8, n)
    step = 1 << 17
    for s in range(0, n, step):
        Xc = X[s:s + step].double()
        cos = (Qd @ Xc.T) / (qn[:, None] * (Xc * Xc).sum(1).sqrt()[None, :])
        sc = tau * cos + (1.0 - tau) / (1.0 + (lq[:, None] - lam[None, s:s + step]).abs())
        v, i = torch.topk(sc, min(kk, sc.shape[1]), dim=1)
        best_s = torch.cat([best_s, v], 1)
        best_i = torch.cat([best_i, i + s], 1)
        v, o = torch.topk(best_s, min(kk, best_s.shape[1]), dim=1)
        best_s, best_i = v, torch.gather(best_i, 1, o)
    best_s, best_i = best_s.cpu().numpy(), best_i.cpu().numpy()
    bad = 0
    for t, hits in enumerate(got):
        # brute-force order: score descending, index ascending inside ties
        order = np.lexsort((best_i[t], -best_s[t]))
        ws, wi = best_s[t][order][:len(hits)], best_i[t][order][:len(hits)]
        gs = np.array([s_ for _, s_ in hits])
        gi = np.array([i_ for i_, _ in hits])
        ok = len(hits) == min(topk, n) and np.allclose(gs, ws, rtol=rtol, atol=0.0)
        if ok and not np.array_equal(gi, wi):
            for a in np.nonzero(gi != wi)[0]:
                # a swapped pair inside a run of equal scores is two summation orders, not a wrong answer
                if not (abs(ws[a] - gs[a]) <= 1e-12 * abs(ws[a]) and gi[a] in best_i[t][np.abs(best_s[t] - ws[a]) <= 1e-12 * abs(ws[a])]):
                    ok = False
        bad += 0 if ok else 1
    return {"n": len(got), "mismatches": bad, "zero_lambda": zero}


def calibrate_eps(X, k, metric="l2", target=2.0, sample=512, seed=5):
    """eps with mean degree before the k-cap ~ target*k; L2 distance or the rectified-cosine
    distance of GRAPH_VARIABLES.md:7."""
    import torch

    n = X.shape[0]
    g = torch.Generator(device=X.device)
    g.manual_seed(seed)
    rows = torch.randperm(n, generator=g, device=X.device)[:sample]
    nn = (X.double() ** 2).sum(1) if n <= (1 << 18) else (X * X).sum(1).double()
    G = X[rows].double() @ X.double().T if n <= (1 << 18) else (X[rows] @ X.T).double()
    if metric == "l2":
        D2 = (nn[rows][:, None] + nn[None, :] - 2 * G).clamp_min(0)
    else:
        D2 = 1.0 - (G / (nn[rows][:, None] * nn[None, :]).sqrt()).clamp(0, 1)
    D2[torch.arange(len(rows), device=X.device), rows] = float("inf")
    kth = int(min(target * k, n - 1))
    vals = torch.topk(D2, kth, dim=1, largest=False).values[:, -1]
    v = float(vals.median().item())
    return v ** 0.5 if metric == "l2" else v


def calibrate_feature_eps(X, k, metric="cosine", target=2.0):
    """Feature mode (SPEC F1-F3): eps with about target*k other columns inside it, from the fp64 Gram of a row sample."""
    import torch

    n, d = X.shape
    Xs = X[:: max(1, n // 65536)].double()
    G = Xs.T @ Xs
    m = G.diagonal()
    if metric == "l2":
        D = (m[:, None] + m[None, :] - 2 * G).clamp_min(0).sqrt() * (n / Xs.shape[0]) ** 0.5
    else:
        D = 1.0 - (G / (m[:, None] * m[None, :]).sqrt()).clamp(0, 1)
    off = D[~torch.eye(d, dtype=torch.bool, device=X.device)]
    return float(torch.quantile(off[: 1 << 24], min(1.0, target * k / max(d - 1, 1))).item())


def run_distribution(kind, n, d, args, device):
    """One unfriendly distribution at the headline shape: build, W + K single-query searches (perturbed items), the
    fallback counters by cause, the scan's operand, and a brute-force check of 32 of the timed queries."""
    import torch

    import pyarrowspace_amd as asp

    X = make_data_torch(kind, n, d, 4242, device)
    if kind == "scaled100":
        # /root/reference/tests/test_3_beir.py:19,190,194-200: unnormalised x100 rows, eps = 10 -- a rectified-cosine distance
        # never exceeds 1, so EVERY item is inside eps: the neighbourhood is the k nearest, the candidate buffers overflow
        metric, kernel, eps = "cosine", "rational", 10.0
    else:
        metric, kernel = args.metric, args.kernel
        eps = calibrate_eps(X, args.k, metric)
    gp = {"eps": eps, "k": args.k, "topk": args.topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    nq = max(args.steps + args.warmup, 64)
    Q = make_queries(X, nq, 43)
    zero = 0

    def go(q):
        try:
            aspace.search(q, gl, args.tau)
            return 0
        except asp.PanicException:
            return 1

    for i in range(args.warmup):
        go(Q[i % nq])
    c0 = aspace.search_counters()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        zero += go(Q[(args.warmup + i) % nq])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c1 = aspace.search_counters()
    asp.enable_search_stats(True)
    us, ops = [], []
    for i in range(min(args.steps, 20)):
        go(Q[(args.warmup + i) % nq])
        us.append(aspace.last_search_stats()["scan_us"])
        ops.append(aspace.last_scan_operand)
    asp.enable_search_stats(False)
    ver = brute_force_verify(aspace, gl, X, [Q[(args.warmup + i) % nq] for i in range(min(32, args.steps))], args.tau, min(args.topk, n))
    out = {"value": args.steps / dt, "unit": "queries/s", "ms_per_step": dt / args.steps * 1e3, "steps": args.steps,
           "zero_lambda": zero, "eps": eps, "metric": metric, "kernel": kernel, "index_build_sec": build_s,
           "fallbacks": {k: c1[k] - c0[k] for k in c1}, "scan_us": float(np.mean(us)), "scan_operands": {o: ops.count(o) for o in set(ops)},
           "verified": ver}
    del aspace, gl, X
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--topk", type=int, default=15)
    ap.add_argument("--tau", type=float, default=0.62)
    ap.add_argument("--eps", type=float, default=0.0, help="0 = calibrate to mean degree 2k")
    ap.add_argument("--metric", choices=["l2", "cosine"], default="l2",
                    help="graph distance: l2 (north_star default) or the rectified cosine of GRAPH_VARIABLES.md:7")
    ap.add_argument("--kernel", choices=["gaussian", "rational"], default="gaussian",
                    help="edge weight: gaussian (north_star default) or 1/(1+(d/sigma)^p) of GRAPH_VARIABLES.md:9")
    ap.add_argument("--lambda-mode", choices=["item", "feature"], default="item",
                    help="item: node energy on the N-node graph; feature: F x F feature Laplacian of TAUMODE.md:8,12-27")
    ap.add_argument("--full", action="store_true",
                    help="measure and check beyond the headline: live PMC traffic passes, kernel-level scan timing, in-distribution "
                         "queries, host threads, batched search, fp64 brute-force verification, unfriendly distributions, the build "
                         "from host memory and the CPU baseline (the --no-* options below switch parts of it off)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the hits of the last timed search (DIR/hit_indices.npy, DIR/hit_scores.npy, float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-queries", type=int, default=24)
    ap.add_argument("--cpu-build-n", type=int, nargs="*", default=[20000, 100000],
                    help="item counts the CPU all-pairs build is timed at (SURVEY section 8d: 20k and 100k)")
    ap.add_argument("--cpu-build-budget", type=float, default=90.0, help="skip a CPU build size predicted to take longer (s)")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="roofline.traffic from profiles/traffic.json (when it is of this workload) instead of two rocprofv3 --pmc passes run now")
    ap.add_argument("--no-threaded", action="store_true", help="skip the 2- and 4-host-thread search runs (kernel-trace profiles: their overlapping kernels stretch each other)")
    ap.add_argument("--no-host-build", action="store_true", help="skip the timing of the reference's own call: build(graph_params, float64 ndarray in HOST memory)")
    ap.add_argument("--no-distributions", action="store_true", help="skip the unfriendly-distribution side keys (isotropic, hierarchical, x100-scaled rows): three more index builds")
    ap.add_argument("--verify-queries", type=int, default=64, help="timed queries (and as many in-distribution ones) re-issued after the timed loops and held against an fp64 brute force on the GPU")
    ap.add_argument("--traffic-probe", action="store_true", help=argparse.SUPPRESS)   # the short child pass live_traffic() profiles
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher around us: be the launcher (nothing in this process has touched the GPU yet, and nothing will)
        sys.exit(launch(args.gpus, sys.argv[1:]))

    live, live_note = None, "not attempted"
    if args.full and "WORLD_SIZE" not in os.environ and not (args.no_live_traffic or args.traffic_probe):
        # before this process touches the GPU: the two counter passes (children under rocprofv3) have the card to themselves
        wl = []
        for name in ("n", "d", "k", "topk", "tau", "eps", "metric", "kernel", "lambda_mode"):
            wl += ["--" + name.replace("_", "-"), str(getattr(args, name))]
        # each pass is a whole build plus a few searches: sized by the build this workload implies (2.6 s at 1M x 768 on
        # the item graph, quadratic in n); beyond two minutes of build per pass the committed profile is the fallback
        build_s = 0.05 if args.lambda_mode == "feature" else 2.6 * (args.n / 1e6) ** 2 * (args.d / 768.0)
        if build_s > 120.0:
            live, live_note = None, "skipped: a counter pass would rebuild the index (%.0f s predicted) twice" % build_s
        else:
            live, live_note = live_traffic(wl, timeout_s=int(150 + 4 * build_s))

    import torch

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; the ranks of the launcher win", file=sys.stderr)
    shared_gpu = int(os.environ.get("ARROWSPACE_BENCH_SHARED_GPU", "0"))     # ranks share this many devices (rehearsal)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    os.environ["ARROWSPACE_DEVICE"] = str(local_rank)
    dist = None
    force_dist = os.environ.get("ARROWSPACE_BENCH_FORCE_DIST", "") not in ("", "0")   # 1-GPU rehearsal of the N>1 path
    if world > 1 or force_dist:
        import torch.distributed as dist_mod

        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")
        if shared_gpu:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group(backend="nccl", device_id=device, rank=rank, world_size=world)

    import pyarrowspace_amd as asp

    n, d = args.n, args.d
    X, centres = make_data(n, d, 42, device, return_centres=True)
    nq_total = max(args.steps + args.warmup, 64)
    Q = make_queries(X, nq_total, 43)
    Qin = make_queries_in_distribution(centres, nq_total, 43)
    if args.eps > 0:
        eps = args.eps
    elif args.lambda_mode == "feature":
        eps = calibrate_feature_eps(X, args.k, args.metric)
    else:
        eps = calibrate_eps(X, args.k, args.metric)
    if dist is not None:
        # every rank derives the same queries and eps from the same seeds; broadcast rank 0's anyway so that
        # a bit-level difference between devices can never desynchronise the ranks' control flow
        qt = torch.from_numpy(Q).to(device)
        et = torch.tensor([eps], dtype=torch.float64, device=device)
        dist.broadcast(qt, 0)
        dist.broadcast(et, 0)
        Q = qt.cpu().numpy()
        eps = float(et.item())
        qt = torch.from_numpy(Qin).to(device)
        dist.broadcast(qt, 0)
        Qin = qt.cpu().numpy()
    gp = {"eps": eps, "k": args.k, "topk": args.topk, "p": 2.0, "sigma": None, "metric": args.metric, "kernel": args.kernel,
          "lambda_mode": args.lambda_mode}
    feature = args.lambda_mode == "feature"

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # ---------------- index build (timed once, inputs resident in HBM)
    single = world == 1 and not force_dist
    Xh32 = None
    # one untimed build of a small index of the same kind first: the process's first pass through the build loads the code
    # object's kernels, sets their attributes and pages the library in (a fresh box measured up to 0.3 s of that inside the
    # graph stage of the first build and none in the second) -- warm-up, as the W untimed searches are for the search
    Xw = make_data(16384, d, 7, device, nclust=64)
    gpw = dict(gp, eps=calibrate_eps(Xw, args.k, args.metric) if not feature else gp["eps"])
    try:
        _w = asp.ArrowSpaceBuilder.build_from_device(gpw, Xw.data_ptr(), "float32", 16384, d, d)
        del _w
    except (ValueError, RuntimeError):   # (a warm-up that cannot be built says nothing about the index)
        pass
    del Xw
    if single:
        barrier()
        t0 = time.perf_counter()
        aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
        barrier()
        build_s = time.perf_counter() - t0
        searcher = lambda q: aspace.search(q, gl, args.tau)  # noqa: E731
        bstats = gl.build_stats()
    else:
        from pyarrowspace_amd import dist as asdist

        b = asdist.shard_bounds(n, world)
        shard = X[b[rank]:b[rank + 1]].clone()      # this rank's rows; the rest arrives by RCCL all-gather
        Xh32 = X.cpu() if args.full and rank == 0 and not args.no_cpu_baseline else None   # (rank 0's CPU baseline scans all N items on the host)
        del X
        torch.cuda.empty_cache()
        barrier()
        t0 = time.perf_counter()
        Index = asdist.HostStagedIndex if shared_gpu else asdist.ShardedIndex
        index = Index.build(gp, shard, dist, force_collectives=force_dist)
        barrier()
        build_s = time.perf_counter() - t0
        searcher = lambda q: index.search(q, args.tau)  # noqa: E731
        aspace = gl = None
        bstats = index.build_stats()
    bt = torch.tensor([build_s], device=device, dtype=torch.float64)
    if dist is not None:
        dist.all_reduce(bt, op=dist.ReduceOp.MAX)
    build_s = float(bt.item())

    # ---------------- search: W warmup + K timed steps
    # CPython's cyclic collector, not the GPU: the first full collection after `import torch` and a build walks everything
    # they left behind -- one search of 32-60 ms, at the 171st staged search exactly, whatever the wall time, with torch's
    # process group alive or destroyed (tools/stall_probe.py; rounds 1-2 blamed the collective layer's watchdog and ran 300
    # untimed "priming" searches to get past it).  A serving process freezes what the build left behind (gc.freeze(): out
    # of the collector's sight, later collections are short) -- so does this one, on every path; no priming searches.
    import gc

    gc.collect()
    gc.freeze()
    primed = 0 if args.traffic_probe else int(os.environ.get("ARROWSPACE_BENCH_PRIME", "0"))   # (A/B knob: tools/prime_ab.sh)
    for i in range(primed):
        searcher(Q[i % len(Q)])
    for i in range(args.warmup):
        searcher(Q[i % len(Q)])
    scan_us = []
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        hits = searcher(Q[(args.warmup + i) % len(Q)])
    barrier()
    dt = time.perf_counter() - t0
    tt = torch.tensor([dt], device=device, dtype=torch.float64)
    if dist is not None:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dt = float(tt.item())
    step_operand = aspace.last_scan_operand if single else index.last_scan_operand()   # what the last timed scan read
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step: the (index, score) hits, score descending
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "hit_indices.npy"), np.array([i for i, _ in hits], dtype=np.float64))
        np.save(os.path.join(args.dump_outputs, "hit_scores.npy"), np.array([s for _, s in hits], dtype=np.float64))
    ranks_seen = world
    if dist is not None:
        # the ranks the collective layer really connected (an all-reduce of ones: RCCL over xGMI, or gloo when the ranks
        # of a rehearsal share a card)
        ones = torch.ones(1, device=device, dtype=torch.float64)
        dist.all_reduce(ones)
        ranks_seen = int(round(float(ones.item())))
    out = {
        "metric": "queries/sec (single-query search, B=1) at N=%dx D=%d fp32; index-build sec alongside" % (n, d),
        "value": args.steps / dt,
        "unit": "queries/s",
        "n_gpus": world,
        "ranks_seen": ranks_seen,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": ("int8 prefilter (items' image) + fp64 exact re-evaluation of every candidate; items fp32 in HBM, API fp64"
                  if step_operand in ("int8", "int8-high") else "f32 prefilter + fp64 exact re-evaluation"),
        "data": "synthetic",
        "config": {"workload": "SURVEY 8(d) synthetic: np.random.default_rng(42) clustered N=%d x D=%d fp32 (1024 centres, noise 0.5, "
                               "rows normalised), k=%d topk=%d tau=%.2f eps=%.5f (calibrated: mean degree ~2k), metric=%s kernel=%s (p=2 is the kernel's "
                               "exponent, GRAPH_VARIABLES.md:9 -- the distance is L2 or rectified cosine, never a general L_p) "
                               "lambda_mode=%s; queries = items perturbed by default_rng(43) noise (deviation from 8(d): a fresh "
                               "sample of the recipe has no neighbour inside eps); BASELINE.json headline config"
                               % (n, d, args.k, args.topk, args.tau, eps, args.metric, args.kernel, args.lambda_mode),
                   "n": n, "d": d, "metric": args.metric, "kernel": args.kernel, "lambda_mode": args.lambda_mode,
                   "parallelism": "row-shard x%d" % world + (" (ranks share %d GPU(s): exchange steps staged through host memory, a "
                                                              "rehearsal of the N-rank job, not a scaling measurement)" % shared_gpu if shared_gpu else "")},
        "parity": PARITY,
        "index_build_sec": build_s,
        "priming_queries": primed,
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(out), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return

    # kernel-level timing of the dominant kernel (scan_dots) with HIP events on its own stream,
    # taken over a second pass so the event reads do not perturb the timed region
    asp.enable_search_stats(True)
    scan_ops = []     # what each of those scans read: the fp32 items, their int8 image, or its high digits alone
    for i in range(min(args.steps, 50)):
        searcher(Q[(args.warmup + i) % len(Q)])
        scan_us.append(aspace.last_search_stats()["scan_us"] if single else index.last_scan_us())
        scan_ops.append(aspace.last_scan_operand if single else index.last_scan_operand())
    scan_ms = float(np.mean(scan_us)) * 1e-3
    scan_operand = max(set(scan_ops), key=scan_ops.count) if scan_ops else ""

    # SURVEY 8(d)'s own query recipe (fresh draws around the index's centres), next to the perturbed-item queries of the
    # headline: same protocol (W warmup + K timed), queries whose lambda_q is 0 -- no item within eps, the reference's
    # assert (src/lib.rs:156-159) -- are skipped and counted, inside the timed region like any other query
    asp.enable_search_stats(False)
    zero_in = 0

    def search_in(q):
        try:
            searcher(q)
            return 0
        except asp.PanicException:
            return 1

    for i in range(args.warmup):
        search_in(Qin[i % len(Qin)])
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        zero_in += search_in(Qin[(args.warmup + i) % len(Qin)])
    barrier()
    tin = torch.tensor([time.perf_counter() - t0], device=device, dtype=torch.float64)
    if dist is not None:
        dist.all_reduce(tin, op=dist.ReduceOp.MAX)
    dt_in = float(tin.item())

    # as_search is re-entrant: T host threads, each issuing B = 1 searches back to back on ONE space -- every
    # call runs on a pooled workspace and stream of its own, one thread's scan under another's finish kernel and host
    # turnaround.  Reported BESIDE the headline (which stays the single-thread, single-query number), never as it.
    threaded = None
    if single and not args.traffic_probe and not args.no_threaded:
        import threading

        threaded = {}
        for nthr in (2, 4):
            per = max(args.steps, 64)
            errs = []

            def worker(t, per=per, nthr=nthr):
                try:
                    for i in range(per):
                        searcher(Q[(args.warmup + t * per + i) % len(Q)])
                except BaseException as e:   # noqa: BLE001 -- reported below, the bench line must still come out
                    errs.append(repr(e))

            ths = [threading.Thread(target=worker, args=(t,)) for t in range(nthr)]
            for t in range(nthr):           # untimed: lets the pool grow to nthr workspaces
                searcher(Q[t % len(Q)])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            dth = time.perf_counter() - t0
            threaded[str(nthr)] = {"value": nthr * per / dth, "unit": "queries/s", "host_threads": nthr, "queries": nthr * per,
                                   "algorithmic_speedup": n * (d + 2) * 4.0 * nthr * per / dth / 1e9 / HBM_PEAK_GBS, "errors": errs[:2]}
        threaded["pool_size"] = aspace.search_pool_size
        threaded["gang_scans_by_members"] = aspace.gang_counters()   # scans that served 1 / 2 / 3 / 4 callers at once
        threaded["note"] = ("\"2\", \"4\": Python threads (the interpreter lock serialises what the threads do between two calls, a wake-up of tens of "
                            "microseconds each); native_*: the same closed loops from native threads against the C ABI (tools/probe/thread_driver.cpp). "
                            "Callers that arrive together share ONE pass over the items (gang scans, DESIGN.md 5.4)")
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import thread_bench

            per = max(args.steps, 64)
            for nthr in (1, 2, 4):
                rate, errs, gangs = thread_bench.native_rate(aspace, gl, Q[args.warmup:], args.tau, nthr, per)
                threaded["native_%d" % nthr] = {"value": rate, "unit": "queries/s", "host_threads": nthr, "queries": nthr * per, "errors": errs,
                                                "scans_by_members": gangs}
        except Exception as e:      # noqa: BLE001 -- a side key must not cost the headline line
            threaded["native_error"] = "%s: %s" % (type(e).__name__, e)

    # extension, reported next to the headline, never as it: batched search, 32 query
    # slots per pass over the items (GEMM-shaped scan on fp32 MFMA)
    batched_qps = batch_pass_ms = None
    batch_dual = 0.0
    if len(Q) >= 64:
        QB = np.ascontiguousarray(np.concatenate([Q[:64]] * 4))    # 256 queries = 8 passes of 32
        # N > 1: the staged batched path (ShardedIndex.search_batch: two collectives per pass of 32 queries)
        run_batch = (lambda: aspace.search_batch(QB, gl, args.tau)) if single else (lambda: index.search_batch(QB, args.tau))
        run_batch()
        dual0 = aspace.batch_dual_scans if single else 0
        tb = []
        for _ in range(7):
            barrier()
            t1 = time.perf_counter()
            run_batch()
            barrier()
            tb.append(time.perf_counter() - t1)
        tbm = torch.tensor([float(np.median(tb))], device=device, dtype=torch.float64)
        if dist is not None:
            dist.all_reduce(tbm, op=dist.ReduceOp.MAX)
        batched_qps = len(QB) / float(tbm.item())
        batch_pass_ms = float(tbm.item()) / (len(QB) / 32) * 1e3
        # (calls of more than 32 queries launch their passes in pairs, and a pair on the int8 images shares ONE scan: scan_gemm_dual_kernel)
        batch_dual = ((aspace.batch_dual_scans - dual0) if single else 0) / (7.0 * len(QB) / 32)   # shared scans per 32-query pass: 0 .. 0.5
    batch_i8 = bool(aspace.last_batch_int8) if single else False

    # ---------------- parity statement about the workload just timed: the first `verify_queries` TIMED queries and as many
    # in-distribution ones, re-issued and held against an fp64 brute force over all items on the GPU (indices and scores)
    verified = None
    if single and not args.traffic_probe and args.verify_queries > 0:
        nv = min(args.verify_queries, args.steps)
        v1 = brute_force_verify(aspace, gl, X, [Q[(args.warmup + i) % len(Q)] for i in range(nv)], args.tau, min(args.topk, n))
        # (in-distribution draws without an item inside eps raise the reference's panic and have no answer to verify: spares)
        v2 = brute_force_verify(aspace, gl, X, [Qin[(args.warmup + i) % len(Qin)] for i in range(min(2 * nv, len(Qin)))], args.tau, min(args.topk, n), want=nv)
        verified = {"n": v1["n"] + v2["n"], "mismatches": v1["mismatches"] + v2["mismatches"],
                    "timed_queries": v1, "in_distribution_queries": v2,
                    "how": "re-issued after the timed loops; torch fp64 cosines of all N items, TAUMODE.md:33 with the library's lambda_q and "
                           "lambdas, top-k by (score desc, index asc); indices equal and scores within 1e-9 relative"}

    # ---------------- unfriendly distributions (side keys, never the headline): same N x D, k, topk, tau; queries = perturbed items
    distributions = None
    if single and not args.traffic_probe and not args.no_distributions and not feature:
        distributions = {}
        for kind in ("isotropic", "hier", "scaled100"):
            try:
                distributions[kind] = run_distribution(kind, n, d, args, device)
            except Exception as e:      # noqa: BLE001 -- a side key must not cost the headline line
                distributions[kind] = {"error": "%s: %s" % (type(e).__name__, e)}

    # ---------------- the reference's own build call: build(graph_params, items: float64 ndarray in HOST memory)
    # (/root/reference/src/lib.rs:271-277) -- the rows stream through two pinned chunks into the ingest kernel (as_build).
    # Beside it: the H2D rate of this box (one pinned 1 GiB copy) and what the device-resident build plus that copy would take.
    build_from_host = None
    if single and not args.traffic_probe and not args.no_host_build:
        try:
            Xh64 = X.cpu().numpy().astype(np.float64)
            pin = torch.empty(1 << 28, dtype=torch.float32).pin_memory()
            dbuf = torch.empty(1 << 28, dtype=torch.float32, device=device)
            dbuf.copy_(pin, non_blocking=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dbuf.copy_(pin, non_blocking=True)
            torch.cuda.synchronize()
            h2d = pin.numel() * 4 / (time.perf_counter() - t0) / 1e9
            del pin, dbuf
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a2, g2 = asp.ArrowSpaceBuilder.build(gp, Xh64)
            torch.cuda.synchronize()
            hb = time.perf_counter() - t0
            same = bool(np.array_equal(a2.lambdas(), aspace.lambdas())) and g2.tau0 == gl.tau0
            st2 = g2.build_stats()
            build_from_host = {"value": hb, "unit": "s", "host_bytes": n * d * 8.0, "h2d_gbs_pinned_measured": h2d, "ingest_sec": st2["ingest_s"],
                               "device_build_plus_copy_sec": build_s + n * d * 8.0 / (h2d * 1e9),
                               "same_lambdas_as_device_build": same,
                               "how": "ArrowSpaceBuilder.build(graph_params, X.astype(float64)) from pageable host memory; two pinned chunks "
                                      "of 64 MB, host threads packing one chunk under the copy of the other and the ingest kernel of the one before"}
            del a2, g2, Xh64
            torch.cuda.empty_cache()
        except Exception as e:      # noqa: BLE001 -- a side key must not cost the headline line
            build_from_host = {"error": "%s: %s" % (type(e).__name__, e)}

    # the scan reads the int8 two-digit image of the items when it can (2 bytes per element + the rows' norm and scale), else fp32
    scan_i8 = scan_operand in ("int8", "int8-high")
    rows_per_gpu = (n + world - 1) // world
    scan_bytes = rows_per_gpu * (d + 2) * 4.0          # N x D fp32 items + N reciprocal norms read, N fp32 dots written
    achieved = scan_bytes / (scan_ms * 1e-3) / 1e9
    d8 = (d + 63) // 64 * 64
    scan_coarse = scan_operand == "int8-high"   # the image's high digits alone: 1 B per element
    scan_moved = rows_per_gpu * ((1.0 if scan_coarse else 2.0) * d8 + 12.0) if scan_i8 else scan_bytes   # bytes the launch moves: image + norms + scales + dots
    if threaded:
        for key in ("2", "4", "native_1", "native_2", "native_4"):
            if key in threaded:
                threaded[key]["frac"] = scan_moved * threaded[key]["value"] / 1e9 / HBM_PEAK_GBS
    # N > 1: every rank's own scan (its rows, its launch time, its operand) next to rank 0's
    per_rank = None
    if dist is not None:
        my_rows = (index.scan_rows[1] - index.scan_rows[0]) if not single else n
        my_moved = my_rows * ((1.0 if scan_coarse else 2.0) * d8 + 12.0) if scan_i8 else my_rows * (d + 2) * 4.0
        mine = {"rank": rank, "rows": int(my_rows), "avg_launch_ms": scan_ms, "operand": scan_operand, "bytes_per_launch": my_moved,
                "achieved": my_moved / (scan_ms * 1e-3) / 1e9, "frac": my_moved / (scan_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
    moved = scan_moved / (scan_ms * 1e-3) / 1e9
    query_bytes = n * (d + 2) * 4.0                      # whole-query algorithmic bytes
    # a 32-query pass: operand + norms + scales + 32 fp16 cosines per row; a pass that shares its scan with its pair's other pass reads half the operand
    batch_moved = (n * (2.0 * d8 * (1.0 - batch_dual) + 8.0 + 64.0) if batch_i8 else query_bytes + n * 64.0) / world
    # Build kernel: bstats["mfma_flops"] counts 2 * (pairs computed) * D -- the fp32-equivalent work.  The default kernel
    # (as_k2bf.hip) issues THREE bf16 products per such flop (head x head, head x tail, tail x head): the roofline
    # fraction is issued bf16 flops / 2.5 PFLOP/s; the fp32-equivalent rate is kept beside it.  ARROWSPACE_K2_FP32=1: the
    # fp32 matrix pipe (157.3 TFLOP/s), one product per flop.
    k2_pipe = aspace.knn_pipe if single else ("fp32" if os.environ.get("ARROWSPACE_K2_FP32", "0") not in ("", "0") else "bf16")
    k2_fp32 = k2_pipe == "fp32"
    mfma_tf_eq = bstats["mfma_flops"] / max(bstats["knn_mfma_s"], 1e-9) / 1e12
    if feature:
        mfma_tf, mfma_peak, build_kernel, build_dtype = mfma_tf_eq, MFMA_F64_PEAK_TF, "gram_f64_kernel", "f64"
    elif k2_fp32:
        mfma_tf, mfma_peak, build_kernel, build_dtype = mfma_tf_eq, MFMA_F32_PEAK_TF, "knn_mfma_dma8_kernel<%s>" % args.metric, "f32"
    elif k2_pipe == "int8":
        # two int8 digits per element, three int8 products per fp32 product: issued int8 ops / 5 POP/s (twice the bf16 rate)
        s16 = os.environ.get("ARROWSPACE_K2_MFMA16", "1") not in ("0",)
        mfma_tf, mfma_peak, build_kernel, build_dtype = (3.0 * mfma_tf_eq, MFMA_I8_PEAK_TOPS, "knn_bf16_kernel<%s, I8%s>" % (args.metric, ", S16" if s16 else ""),
                                                         "int8 two-digit image (3 products per fp32 product, exact int32 accumulation) on %s"
                                                         % ("v_mfma_i32_16x16x64_i8" if s16 else "v_mfma_i32_32x32x32_i8"))
    else:
        mfma_tf, mfma_peak, build_kernel, build_dtype = 3.0 * mfma_tf_eq, MFMA_BF16_PEAK_TF, "knn_bf16_kernel<%s>" % args.metric, "bf16 head + tail (3 products per fp32 product)"

    # HBM-side traffic per launch: PMC counters need rocprofv3 around the process -- measured by live_traffic() in two
    # child passes at the start of this run; when that was not possible (no rocprofv3, --no-live-traffic, N > 1) taken
    # from the committed profile of the same workload, profiles/traffic.json (profiles/collect.sh), and labelled so;
    # null for any other workload
    traffic_scan = traffic_mfma = traffic_batch = None
    traffic_source = None
    k2_fp32_env = os.environ.get("ARROWSPACE_K2_FP32", "0") not in ("", "0")
    # rows up to 1024 floats take the LDS-DMA ring scan, wider rows the register-staged one
    scan_kernel = "scan_dma_kernel" if d <= 1024 and os.environ.get("ARROWSPACE_SCAN_VARIANT", "0") in ("", "0") else "scan_dots_f32_kernel"
    if scan_coarse:
        scan_kernel = "scan_tile_kernel"   # (the coarse operand lies in tiles of 64 rows x 16 columns: as_scan.hip)
    # (the name the rocprofv3 summaries under profiles/ carry: rows of 256 columns and more run the tile scan with its dynamic chunk schedule)
    # (... and three chunks of 64 rows per wave or more: launch_scan in as_scan.hip)
    waves = 4 * min(max(n // world // 128, 1), 2 * torch.cuda.get_device_properties(device).multi_processor_count)
    scan_kernel_name = ("scan_tile_kernel_dyn" if scan_coarse and d8 // 16 >= 16 and n // world >= waves * 64 * 3
                        and os.environ.get("ARROWSPACE_TILE_DYN", "1") != "0" else scan_kernel)
    if live:
        traffic_scan, traffic_mfma, traffic_batch = live.get(scan_kernel), (live.get("knn_mfma_kernel") if k2_fp32_env else live.get("knn_bf16_kernel")), (live.get("scan_gemm_dual_kernel") if batch_dual > 0 else None) or live.get("scan_gemm_kernel")
        traffic_source = live_note
    else:
        try:
            tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
            if tj["workload"] == {"n": n, "d": d} and world == 1 and args.metric == "l2" and not feature:
                traffic_scan = tj.get(scan_kernel, {}).get("bytes_per_launch")
                traffic_mfma = tj.get("knn_mfma_kernel" if k2_fp32_env else "knn_bf16_kernel", {}).get("bytes_per_launch")
                traffic_batch = tj.get("scan_gemm_dual_kernel" if batch_dual > 0 else "scan_gemm_kernel", {}).get("bytes_per_launch")
                traffic_source = ("profiles/traffic.json (rocprofv3 --pmc passes of this workload, profiles/collect.sh); live passes: %s"
                                  % live_note)
        except (OSError, KeyError, ValueError):
            pass

    out.update({
        "verified": verified,
        "distributions": distributions,
        "in_distribution_queries": {"value": (args.steps - zero_in) / dt_in if dt_in > 0 else None, "unit": "queries/s",
                                    "ms_per_step": dt_in / args.steps * 1e3, "steps": args.steps, "zero_lambda_skipped": zero_in,
                                    "frac": scan_moved / (dt_in / args.steps) / 1e9 / HBM_PEAK_GBS,
                                    "algorithmic_speedup": query_bytes / world / (dt_in / args.steps) / 1e9 / HBM_PEAK_GBS,
                                    "workload": "SURVEY 8(d) query recipe: the index's 1024 centres, labels and noise 0.5 from "
                                                "np.random.default_rng(43), rows normalised"},
        "index_build_from_host_sec": None if not build_from_host or "value" not in build_from_host else build_from_host["value"],
        "index_build_from_host": build_from_host,
        "batched_queries_per_sec": batched_qps,
        "threaded_queries_per_sec": threaded,
        "zero_lambda_rate": zero_in / args.steps,
        # single-query searches of this run that needed a second pass over the items, by cause (as_search_counters)
        "fallback_rate": (lambda c: None if c is None else dict(c, rate=c["searches_with_rerun"] / max(c["searches"], 1)))(
            aspace.search_counters() if single else None),
        "build_stages_sec": {k: bstats[k] for k in ("ingest_s", "knn_mfma_s", "refine_s", "fallback_s", "graph_s")},
        "build_fallback_rows": bstats["fallback_rows"],
        "build_band_rows": bstats["band_rows"],
        # `achieved`, `frac`: the bytes one launch MOVES (operand image + norms + scales read, dots written; `traffic` is the
        # PMC measurement of the same) over the launch's duration, against the 8 TB/s peak -- a roofline fraction, <= 1.
        # SURVEY 8(d)'s ALGORITHMIC bytes N (D + 2) 4 (an fp32 scan of the items) over the same time is kept beside it as
        # `algorithmic_speedup`: how many fp32-scan rooflines the launch is worth (above 1 when it reads the 1- or 2-byte image).
        "roofline": {"kernel": scan_kernel_name, "bound": "hbm", "achieved": moved, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": moved / HBM_PEAK_GBS, "traffic": traffic_scan,
                     "frac_from_traffic": None if traffic_scan is None else traffic_scan / (scan_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                     "traffic_source": traffic_source if traffic_scan is not None else "none (live passes: %s)" % live_note,
                     "avg_launch_ms": scan_ms, "bytes_per_launch": scan_moved,
                     "operand": ("int8 image, high digits alone (1 B per element; every candidate re-evaluated exactly)" if scan_coarse
                                 else "int8 two-digit image (2 B per element)") if scan_i8 else "fp32 items",
                     "algorithmic_bytes_per_launch": scan_bytes, "algorithmic_gbs": achieved, "algorithmic_speedup": achieved / HBM_PEAK_GBS,
                     "note": "this launch also collects the scorer's candidates (fused tail, DESIGN.md 5.4); ARROWSPACE_SCAN_FP32=1 scans "
                             "the fp32 items (round 3's operand), ARROWSPACE_NO_FUSED_TAIL=1 runs the plain kernel"},
        "roofline_per_rank": per_rank,
        "roofline_query": {"bound": "hbm", "achieved": scan_moved / (dt / args.steps) / 1e9, "peak": HBM_PEAK_GBS,
                           "unit": "GB/s", "frac": scan_moved / (dt / args.steps) / 1e9 / HBM_PEAK_GBS,
                           "algorithmic_speedup": query_bytes / world / (dt / args.steps) / 1e9 / HBM_PEAK_GBS,
                           "note": "whole query, host-visible latency, per GPU: the scan's bytes moved over ms_per_step"},
        "roofline_batch": None if batch_pass_ms is None else {
            "kernel": ("scan_gemm_dual_kernel" if batch_dual > 0 else "scan_gemm_kernel") + " + per-slot selection", "bound": "hbm", "queries_per_pass": 32,
            "queries_per_scan": 32.0 / (1.0 - batch_dual), "shared_scans_per_pass": batch_dual,
            "achieved": batch_moved / (batch_pass_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": batch_moved / (batch_pass_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "ms_per_pass": batch_pass_ms,
            "bytes_per_pass": batch_moved, "traffic": traffic_batch,
            "operand": "int8 two-digit images of items and queries (2 B per element)" if batch_i8 else "fp32 items as bf16 head + tail",
            "algorithmic_speedup": query_bytes / world / (batch_pass_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "note": "whole 32-query pass, host-visible, per GPU; `frac`: the bytes the pass moves (operand -- HALF of it where two passes "
                    "share one scan, `shared_scans_per_pass` = 0.5 --, norms, 32 fp16 cosines per row; `traffic`: per LAUNCH, which then "
                    "serves 64 queries) against the peak; `algorithmic_speedup`: SURVEY 8(d)'s N*(D+2)*4 per pass over the same time.  int8 "
                    "operand: three v_mfma_i32_32x32x32_i8 products per column, exact int32 sums; bf16 operand (the items' or the queries' "
                    "quantisation error too large, ARROWSPACE_SCAN_FP32=1): three bf16 products.  Either way the pass only prefilters: its "
                    "error bound sits in the prefilter's and the proof's coefficients (DESIGN.md 5.5).  ARROWSPACE_BATCH_F32_DOTS=1 is the "
                    "fp32 form"},
        "roofline_build": {"kernel": build_kernel, "bound": "mfma", "achieved": mfma_tf, "peak": mfma_peak,
                           "unit": "TOP/s" if k2_pipe == "int8" and not feature else "TFLOP/s", "frac": mfma_tf / mfma_peak, "traffic": traffic_mfma,
                           "flops_issued": (1.0 if feature or k2_fp32 else 3.0) * bstats["mfma_flops"], "kernel_sec": bstats["knn_mfma_s"],
                           "fp32_equivalent_tflops": mfma_tf_eq, "fp32_equivalent_flops": bstats["mfma_flops"],
                           "frac_of_fp32_mfma_peak": mfma_tf_eq / MFMA_F32_PEAK_TF, "dtype": build_dtype,
                           "pipe": "f64" if feature else k2_pipe,
                           "note": "k-NN kernels of the build (threshold pass + symmetric pass: half the distance block); the "
                                   "pipe only prefilters -- graphs are bit-identical on int8, bf16 and fp32 (DESIGN.md 5.2)"},
    })

    # ---------------- CPU baseline: the oracle (fp64 C/OpenMP restatement) on this box's host cores, rank 0 (at any N)
    lam_all = deg_all = None
    if not single and not args.no_cpu_baseline and not feature:
        lam_all = index.lambdas()        # (collectives: every rank takes part, rank 0 uses the result)
        deg_all = index.degrees()
    if rank == 0 and not args.no_cpu_baseline and (single or (Xh32 is not None and lam_all is not None)):
        from oracle import oracle_c

        cores = oracle_c.threads()
        Xh = X.double().cpu().numpy() if single else Xh32.double().numpy()
        nq = args.cpu_queries
        if feature:
            # feature mode: the CPU build is N-linear (Gram + per-item energies) -- timed on the whole index
            t0 = time.perf_counter()
            ref = oracle_c.OracleIndex(Xh, gp)
            cpu_build = [{"value": time.perf_counter() - t0, "unit": "s", "n": n, "sample": "full feature-mode build (fp64 Gram + energies)"}]
        elif single:
            ref = oracle_c.OracleSearchOnly(Xh, gp, gl.degrees(), aspace.lambdas(), gl.tau0)
            cpu_build = None
        else:
            ref = oracle_c.OracleSearchOnly(Xh, gp, deg_all, lam_all, index.engine.tau0())
            cpu_build = None
        ref.search(Q[0], args.tau, fused=True)
        cpu_hits = []
        t0 = time.perf_counter()
        for i in range(nq):
            cpu_hits.append(ref.search(Q[(args.warmup + i) % len(Q)], args.tau, fused=True))
        cpu_dt = time.perf_counter() - t0
        del ref
        # the checker's answers to those queries, held against the GPU path's (indices rank-exact, scores to 1e-9): free here
        agree = None
        if single:
            agree = 0
            for i, (want, _) in enumerate(cpu_hits):
                got = searcher(Q[(args.warmup + i) % len(Q)])
                agree += int([a for a, _ in got] == [a for a, _ in want]
                             and np.allclose([b for _, b in got], [b for _, b in want], rtol=1e-9, atol=0.0))
        if cpu_build is None:
            # all-pairs fp64 build: N^2 work, timed at the sizes SURVEY 8(d) names, never extrapolated into `value`
            cpu_build, per_pair = [], None
            for nb in sorted(set(min(v, n) for v in args.cpu_build_n)):
                if per_pair is not None and per_pair * nb * nb > args.cpu_build_budget:
                    cpu_build.append({"value": None, "unit": "s", "n": nb, "sample": "skipped: predicted %.0f s from the smaller size"
                                      % (per_pair * nb * nb)})
                    continue
                t0 = time.perf_counter()
                oracle_c.OracleIndex(Xh[:nb], gp)
                tb_ = time.perf_counter() - t0
                per_pair = tb_ / (nb * nb)
                cpu_build.append({"value": tb_, "unit": "s", "n": nb, "sample": "all-pairs fp64 build on the first %d rows (cache-blocked tiles of 8 rows, AVX2 / AVX-512)" % nb})
        out["cpu_baseline"] = {
            "value": nq / cpu_dt, "unit": "queries/s", "cores": cores, "kind": "port",
            "sample": "%d single queries over the full N=%d x D=%d fp64 items; one fused pass per query (neighbour search and "
                      "cosines from the same read of the items, scorer over the kept cosines), OpenMP static over items, items "
                      "first-touched by the threads that scan them; %.2f GB/s effective" % (nq, n, d, n * d * 8.0 * nq / cpu_dt / 1e9),
            "gpu_agrees_on_those_queries": None if agree is None else "%d/%d" % (agree, nq),
            "index_build": cpu_build,
        }
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    if verified is not None and verified["mismatches"]:
        print("bench.py: %d of %d verified queries differ from the fp64 brute force" % (verified["mismatches"], verified["n"]), file=sys.stderr)
        sys.exit(3)


if __name__ == "__main__":
    main()
