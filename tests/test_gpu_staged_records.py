"""GPU: the two record merges that end a row-sharded search, on hand-built records through the staged C ABI.
as_query_lambda / as_query_lambda_batch (q_lambda_kernel) rank up to 1 024 all-gathered as_knn_rec by (key, id), keep the k
best valid ones and form lambda_q from their dist / gy / deg / ny; as_query_finish / as_query_finish_batch
(hits_final_kernel) rank up to 8 208 as_hit_rec by (score descending, id ascending), OR the flag records (id -2) into the
exactness and overflow flags and publish the answer.  The end-to-end tests (test_gpu_dist.py, test_gpu_multirank.py,
test_gpu_wide_k.py) feed them what the scans of clustered data leave: trailing empties, no ties at the cut, no flag, a few
dozen hit records.  Here the records are made by hand -- empties anywhere with hostile payloads, ties across rank blocks
at the cut, ids up to 1e9, every flag bit, both capacities, the degenerate lambdas -- and every outcome is compared with
oracle_np.staged_lambda / staged_merge: what the merges select or copy exactly, lambda_q to RTOL, and bit for bit where
only the layout of the same records changes.  The k-NN records come from VIRTUAL items (vectors with chosen ids and
degrees; oracle_np.pair_quantities gives key / dist / gy / ny, so the fields are consistent): the lambda step reads only
the records, |q|^2 and the graph's sigma, p, tau0.  tests/test_staged_records_inputs.py checks the inputs' conditioning
on the oracle alone."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from conftest import calibrate_eps, clustered
from oracle import oracle_np
from test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu

AS_OK, AS_EZEROLAMBDA, AS_EUNSUPPORTED = 0, 2, 4
REC_CAP, HIT_CAP = 1024, 8208            # as_record_capacity(0 / 1)
SLOTS = 32                               # as_query_slots of a batched workspace
TAU = 0.62

#           n     d   k    topk  metric    kernel      p    sigma  R (rank blocks of the every-slot-valid case)
CONFIGS = {
    "k1":    (64,   24, 1,   4,    "l2",     "gaussian", 2.0, None, 1),
    "k5":    (64,   24, 5,   15,   "cosine", "rational", 2.0, None, 2),
    "k7p":   (96,   24, 7,   1,    "l2",     "rational", 1.5, 0.6,  3),     # p != 2, explicit sigma
    "k63":   (128,  24, 63,  15,   "l2",     "gaussian", 2.0, None, 3),
    "k64":   (128,  24, 64,  64,   "cosine", "rational", 2.0, None, 2),     # 64 / 65: the second candidate per lane
    "k65":   (128,  24, 65,  15,   "l2",     "gaussian", 2.0, None, 2),
    "k120":  (300,  24, 120, 15,   "l2",     "gaussian", 2.0, None, 8),     # 8 x 120 = 960: the design point
    "k120c": (300,  24, 120, 15,   "cosine", "rational", 2.0, None, 8),
    "cap":   (1100, 16, 6,   1024, "l2",     "gaussian", 2.0, None, 8),     # hit-merge capacity: 8 x 1 025
}
LAMBDA_CONFIGS = [c for c in CONFIGS if c != "cap"]


# ------------------------------------------------------------------------------------------------ inputs (numpy only)
def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


@functools.lru_cache(maxsize=None)
def config_data(name):
    """-> (items, graph_params) of a config."""
    n, d, k, topk, metric, kernel, p, sigma, _ = CONFIGS[name]
    X = clustered(n, d, nclust=4, seed=100 + k)
    if metric == "cosine":
        # positive orthant: every cosine is positive.  With mixed signs a third of the pairs sit at the rectified distance 1.0
        # exactly, and a k = 120 list on 300 items ends inside that tie: no path can prove such a list, and the workspace would
        # carry the scan's own inexact flag into every merge
        X = np.abs(X)
    gp = {"eps": calibrate_eps(X, min(k, n // 3), metric), "k": k, "topk": topk, "p": p, "sigma": sigma, "metric": metric, "kernel": kernel}
    return X, gp


def prm_of(name):
    return oracle_np.resolve_params(config_data(name)[1])


def case_query(name, row=3):
    """A query on the 2^-8 grid: |q|^2 and, under l2, every key of a virtual item q + e (e on the grid) are exact in fp64
    whatever the summation order, so equal keys are equal bit for bit."""
    q = np.round(config_data(name)[0][row] * 256.0) / 256.0
    assert float(q @ q) > 0.25
    return np.ascontiguousarray(q)


def id_bits(ids):
    return np.asarray(ids, dtype=np.int64).view(np.float64)


def distinct_ids(rng, count, top=10 ** 9):
    """count distinct ids in [0, top], in random order; 0 and top among them when there is room."""
    out = np.unique(rng.integers(1, top, size=2 * count + 16))
    rng.shuffle(out)
    out = out[:count].astype(np.int64)
    if count >= 4:
        out[0], out[1] = top, 0
        rng.shuffle(out)
    return out


def to_records(prm, q, Xv, ids, deg):
    """as_knn_rec of virtual items Xv against q."""
    Xv = np.asarray(Xv, dtype=np.float64).reshape(-1, len(q))
    nq, n = float(q @ q), np.einsum("ij,ij->i", Xv, Xv)
    key, dist, gy = oracle_np.pair_quantities(q, Xv, nq, n, prm["metric"])
    rec = np.empty((len(Xv), 6))
    rec[:, 0] = id_bits(ids)
    rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4] = key, dist, gy, deg
    rec[:, 5] = n if prm["metric"] == oracle_np.METRIC_L2 else np.where(n > 0, 1.0, 0.0)
    return rec


def empties(count):
    """Empty slots (id -1) with hostile payloads: keys 0.0, -1.0, +inf, NaN; NaN dist / gy; infinite degree."""
    rec = np.empty((count, 6))
    rec[:, 0] = id_bits(np.full(count, -1))
    rec[:, 1] = np.array([0.0, -1.0, np.inf, np.nan])[np.arange(count) % 4]
    rec[:, 2] = rec[:, 3] = np.nan
    rec[:, 4], rec[:, 5] = np.inf, -1.0
    return rec


def make_valid(prm, q, rng, nvalid, k, run=1, qtwin=False):
    """nvalid virtual items q + e (e on the 2^-8 grid, about sigma away) as records, ids distinct and random.  run > 1: `run`
    items share one key exactly, placed so that the k-th place falls inside the run (l2: q + e, q - e and q + roll(e); cosine:
    x, 2 x, 4 x -- equal cosines), with different degrees (l2: also different gy and ny).  qtwin: one item IS the query.
    -> (records, indices of the run's members)."""
    if nvalid < max(run, 1) or nvalid == 0:
        run = 1
    if nvalid == 0:
        return np.zeros((0, 6)), []
    l2 = prm["metric"] == oracle_np.METRIC_L2
    d, nbase = len(q), nvalid - (run - 1)
    r = prm["sigma"] if l2 else np.sqrt(2.0 * prm["sigma"])
    A = max(2, int(256.0 * r / np.sqrt(d)))
    E = rng.integers(-A, A + 1, size=(nbase, d)).astype(np.float64)
    E[(E == 0).all(axis=1), 0] = 1.0
    Xv = q[None, :] + E / 256.0
    if qtwin:
        Xv[0] = q
    deg = rng.uniform(0.3, 6.0, size=nvalid)
    members = []
    if run > 1:
        key = oracle_np.pair_quantities(q, Xv, float(q @ q), np.einsum("ij,ij->i", Xv, Xv), prm["metric"])[0]
        anchor = int(np.lexsort((np.arange(nbase), key))[min(max(0, k - run + 1), nbase - 1)])
        x = Xv[anchor]
        twins = [q - (x - q), q + np.roll(x - q, 1)] if l2 else [2.0 * x, 4.0 * x]
        Xv = np.vstack([Xv] + twins[: run - 1])
        members = [anchor] + list(range(nbase, nvalid))
        deg[members] = np.array([0.35, 5.5, 2.0])[:run]
    return to_records(prm, q, Xv, distinct_ids(rng, nvalid), deg), members


def scatter(valid, R, per, rng, members=()):
    """R rank blocks of `per` slots: the valid records at random slots anywhere, the run's members in different blocks,
    hostile empties everywhere else.  -> (R * per, 6)."""
    m = R * per
    assert len(valid) <= m
    out = empties(m)
    taken = []
    for j, _ in enumerate(members):
        blk = j % R
        free = [s for s in range(blk * per, (blk + 1) * per) if s not in taken] or [s for s in range(m) if s not in taken]
        taken.append(int(free[rng.integers(len(free))]))
    tk = set(taken)
    rest = [int(s) for s in rng.permutation(m) if int(s) not in tk][: len(valid) - len(members)]
    others = [i for i in range(len(valid)) if i not in set(members)]
    if taken:
        out[taken] = valid[list(members)]
    if rest:
        out[rest] = valid[others]
    return out


@functools.lru_cache(maxsize=None)
def lambda_cases(name):
    """The single-form cases of a config: dicts name / recs (m x 6) / m / zero (a degenerate lambda) / tie (the k-th
    place lies inside a run of equal keys)."""
    n, d, k, topk, metric, kernel, p, sigma, R = CONFIGS[name]
    prm, q, rng = prm_of(name), case_query(name), _rng("lambda", name)
    cases = []

    def add(cname, recs, zero=False, m=None, tie=False):
        cases.append(dict(name=cname, recs=recs, m=len(recs) if m is None else m, zero=zero, tie=tie))

    add(f"every_slot_valid_R{R}", scatter(make_valid(prm, q, rng, R * k, k)[0], R, k, rng))
    if name == "k64":
        add("capacity_1024", scatter(make_valid(prm, q, rng, REC_CAP, k)[0], REC_CAP // k, k, rng))
    if k > 1:
        add("fewer_than_k", scatter(make_valid(prm, q, rng, k - 1, k)[0], 3, k, rng))
    add("exactly_k", scatter(make_valid(prm, q, rng, k, k)[0], 3, k, rng))
    add("many_more_than_k", scatter(make_valid(prm, q, rng, min(3 * k + 5, 5 * k - 3), k)[0], 5, k, rng))
    Rt = (2 * k + 7) // k + 1
    for cname, run in (("tie_pair_at_the_cut", 2), ("tie_run_of_3_across_the_cut", 3)):
        v, mem = make_valid(prm, q, rng, k + 6, k, run=run)
        add(cname, scatter(v, Rt, k, rng, mem), tie=True)
    add("item_identical_to_the_query", scatter(make_valid(prm, q, rng, k + 3, k, qtwin=True)[0], Rt, k, rng))
    # the degenerate outcomes: lambda_q == 0
    add("m_0", empties(1), zero=True, m=0)
    add("all_slots_empty", empties(2 * k), zero=True)
    if metric == "l2" and kernel == "gaussian":
        u = rng.standard_normal((min(k, 4), d))
        far = q[None, :] + 60.0 * prm["sigma"] * u / np.linalg.norm(u, axis=1, keepdims=True)       # exp(-1800) == 0
        add("weights_underflow", scatter(to_records(prm, q, far, distinct_ids(rng, len(far)), rng.uniform(0.3, 6.0, len(far))), 2, k, rng), zero=True)
    c = min(k, 3)       # c copies of q, each of degree c - 1: deg_q = c = deg_j + a_j, alpha == beta, dist == 0 -> every edge energy 0
    add("edge_energies_zero", scatter(to_records(prm, q, np.tile(q, (c, 1)), distinct_ids(rng, c), np.full(c, c - 1.0)), 2, k, rng), zero=True)
    return cases


def ranked(recs):
    """Indices of the valid records in (key, id) order."""
    ids = oracle_np.rec_ids(recs)
    ok = np.nonzero(ids >= 0)[0]
    return ok[np.lexsort((ids[ok], recs[ok, 1]))]


def wrong_pick(recs, k):
    """The records with the ids of the k-th and the (k+1)-th ranked record exchanged: the merge then keeps the payload
    a wrong tie-break (the higher id) would have kept."""
    o = ranked(recs)
    out = recs.copy()
    out[o[k - 1], 0], out[o[k], 0] = recs[o[k], 0], recs[o[k - 1], 0]
    return out


def permuted_blocks(recs, per, rng):
    """The same records with the rank blocks in another order and every block's slots in another order."""
    b = recs.reshape(-1, per, recs.shape[1])
    b = b[rng.permutation(b.shape[0])]
    return np.concatenate([blk[rng.permutation(per)] for blk in b])


def batch_lambda_case(name, nranks, nb=29):
    """Records [nranks][SLOTS][k] of a batched pass: slot b < nb has its own query, its own number of valid records (all
    different; 0, k and k + 1 among them) and its own tie pattern (none / pair / run of 3, at the cut where the slot has
    more than k records); slots >= nb are empty.  -> (queries, records, per-slot records flattened in rank order)."""
    k = CONFIGS[name][2]
    prm, rng = prm_of(name), _rng("batch", name, nranks)
    m = nranks * k
    counts = [c for c in rng.permutation(m + 1) if c not in (0, k, min(k + 1, m))][: nb - 3]
    counts = [0, k, min(k + 1, m)] + [int(c) for c in counts]
    while len(counts) < nb:
        counts.append(int(rng.integers(1, m + 1)))
    counts = [counts[i] for i in rng.permutation(nb)]
    Q = np.stack([case_query(name, row=b) for b in range(nb)])
    recs = np.empty((nranks, SLOTS, k, 6))
    flat = []
    for b in range(SLOTS):
        if b < nb:
            v, mem = make_valid(prm, Q[b], rng, counts[b], k, run=1 + b % 3)
            f = scatter(v, nranks, k, rng, mem)
        else:
            f = empties(m)
        flat.append(f)
        recs[:, b] = f.reshape(nranks, k, 6)
    return Q, recs, flat, counts


# ---- hit records
HIT_KINDS = ("plain", "fewer_than_topk", "tie_at_the_cut", "tie_run_across_the_cut", "all_scores_equal", "signed_zeros", "minus_inf_valid")


def hit_case(kind, topk, m, R, rng, flags=()):
    """m as_hit_rec in R blocks: valid records with ids up to 1e9, one id -2 record per entry of `flags` (in a non-first
    block where there is one), id -1 slots carrying +inf or NaN everywhere else."""
    per = m // max(R, 1)
    rec = np.empty((m, 2))
    rec[:, 0] = id_bits(np.full(m, -1))
    rec[:, 1] = np.where(np.arange(m) % 3 == 0, np.nan, np.inf)
    slots = [int(s) for s in rng.permutation(m)]
    fpos = [s for s in slots if s >= per or R == 1][: len(flags)]
    for s, f in zip(fpos, flags):
        rec[s, 0], rec[s, 1] = id_bits([-2])[0], float(f)
    fset = set(fpos)
    free = [s for s in slots if s not in fset]
    nv = {"fewer_than_topk": topk // 2, "minus_inf_valid": min(topk, len(free))}.get(kind, len(free))
    pos = np.array(sorted(free[:nv]), dtype=np.int64)
    sc = rng.standard_normal(nv)
    if kind == "all_scores_equal":
        sc[:] = 0.25
    elif kind == "signed_zeros":
        sc = np.where(np.arange(nv) % 3 == 0, sc, np.where(np.arange(nv) % 3 == 1, 0.0, -0.0))
    elif kind == "minus_inf_valid":
        sc[rng.permutation(nv)[: (nv + 2) // 3]] = -np.inf
    elif kind in ("tie_at_the_cut", "tie_run_across_the_cut") and nv > topk:
        o = np.argsort(-sc, kind="stable")
        a = o[topk - 1]
        for j in range(topk, nv):                      # the other side of the cut comes from another block where there is one
            if pos[o[j]] // per != pos[a] // per:
                sc[o[j]], sc[o[topk]] = sc[o[topk]], sc[o[j]]
                break
        o = np.argsort(-sc, kind="stable")
        lo, hi = (topk - 1, topk + 1) if kind == "tie_at_the_cut" else (max(0, topk - 2), min(nv, topk + 2))
        sc[o[lo:hi]] = sc[o[topk - 1]]
    rec[pos, 0] = id_bits(distinct_ids(rng, nv))
    rec[pos, 1] = sc
    return rec


def flags_expected(fl):
    """as_query_flags after a merge that OR-ed the bits fl: (knn_inexact, score_inexact)."""
    return (1 if fl & 1 else 0) | (2 if fl & 4 else 0), (1 if fl & 2 else 0) | (2 if fl & 8 else 0)


# ------------------------------------------------------------------------------------------------ driving the steps
STATS = {"dev": {}, "exact": 0}


def exact(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b), (a, b)
    STATS["exact"] += max(int(a.size), 1)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


class Steps:
    """One index in one process (ShardedIndex.build on one rank) and its engine's staged calls; records go up as torch
    tensors, the two merges are called on the library directly so that m and the status stay visible."""

    def __init__(self, name, extra=None):
        import torch
        from pyarrowspace_amd.dist import ShardedIndex
        self.torch, self.name = torch, name
        X, gp = config_data(name)
        self.X, self.gp = X, dict(gp, **(extra or {}))
        self.n, self.d, self.k, self.topk = X.shape[0], X.shape[1], gp["k"], min(gp["topk"], X.shape[0])
        self.index = ShardedIndex.build(self.gp, torch.from_numpy(X).cuda())
        self.e = self.index.engine
        self.L = self.e.L
        self.prm = oracle_np.resolve_params(self.gp)
        self.tau0 = self.e.tau0()
        feature = self.gp.get("lambda_mode") == "feature"                   # (a feature-mode workspace keeps one k-NN record)
        assert (feature or self.e.k == self.k) and self.e.hcap == self.topk + 1      # the record strides the batched layouts are built on
        self.keep = []
        self.batch = False
        self.good_hits = hit_case("plain", self.topk, 2 * (self.topk + 1), 2, _rng("good", name))

    def up(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        t = self.torch.from_numpy(a if a.size else np.zeros((1, a.shape[-1]))).cuda()
        self.torch.cuda.synchronize()
        self.keep.append(t)
        return t

    def scan_only(self, q, mode=0):
        self.q = np.ascontiguousarray(q, dtype=np.float64)
        self.e.set_mode(mode)
        self.e.query_scan(self.q, 0, self.n)
        self.torch.cuda.synchronize()

    def scan(self, q):
        """Scan the whole space for q and take the scan's own records through the steps; where the fast path cannot prove its
        lists exact, escalate as ShardedIndex.search does (dist.next_mode).  Leaves a workspace with clean flags, and the
        answer of that pass in scan_fin.  ONE score per scan, here and everywhere in this file: the scorer appends its
        candidates behind those of the previous call until a scan resets the count (the merges may be repeated at will)."""
        from pyarrowspace_amd.dist import next_mode
        mode = 0
        while mode is not None:
            self.scan_only(q, mode)
            exact(self.lam_own(), AS_OK)
            self.score(TAU)
            self.scan_fin = fin = self.finish()
            mode = next_mode(mode, bool((fin["ki"] | fin["si"]) & 1), (1 if fin["ki"] & 2 else 0) | (2 if fin["si"] & 2 else 0))
        exact([fin["ki"], fin["si"]], [0, 0])

    def lam(self, recs, m=None):
        t = self.up(recs)
        st = self.L.as_query_lambda(self.e.q, C.c_void_p(t.data_ptr()), len(recs) if m is None else m)
        self.torch.cuda.synchronize()
        return st

    def lam_own(self):
        st = self.L.as_query_lambda(self.e.q, C.c_void_p(self.e.knn_local.data_ptr()), self.k)
        self.torch.cuda.synchronize()
        return st

    def score(self, tau=TAU):
        self.e.query_score(tau)
        self.torch.cuda.synchronize()

    def finish(self, hits=None, m=None):
        """-> dict st / n / ids / sbits (score bit patterns) / lq / ki / si (as_query_flags)."""
        if hits is None:
            t, m = self.e.hits_local, self.topk + 1
        else:
            t, m = self.up(hits), (len(hits) if m is None else m)
        idx, sc = np.full(max(self.topk, 1), -7, dtype=np.int64), np.full(max(self.topk, 1), np.nan)
        ln, lq, ki, si = C.c_int64(-7), C.c_double(-7.0), C.c_int32(-7), C.c_int32(-7)
        st = self.L.as_query_finish(self.e.q, C.c_void_p(t.data_ptr()), m, idx.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p),
                                    C.byref(ln), C.byref(lq))
        self.L.as_query_flags(self.e.q, C.byref(ki), C.byref(si))
        self.torch.cuda.synchronize()
        self.keep.clear()
        n = max(int(ln.value), 0)
        return dict(st=st, n=int(ln.value), ids=idx[:n].copy(), sbits=bits(sc[:n]).copy(), lq=float(lq.value), ki=ki.value, si=si.value)

    def lambda_of(self, recs, m=None):
        """The lambda step on `recs`, read back through a finish on valid hit records: (status of the step, finish)."""
        st = self.lam(recs, m)
        return st, self.finish(self.good_hits)

    def as_search(self, q, tau):
        idx, sc = np.zeros(max(self.topk, 1), dtype=np.int64), np.zeros(max(self.topk, 1))
        ln, lq = C.c_int64(0), C.c_double(0.0)
        q = np.ascontiguousarray(q, dtype=np.float64)
        st = self.L.as_search(self.e.sp, self.e.gr, q.ctypes.data_as(C.c_void_p), q.shape[0], float(tau), idx.ctypes.data_as(C.c_void_p),
                              sc.ctypes.data_as(C.c_void_p), C.byref(ln), C.byref(lq))
        self.torch.cuda.synchronize()
        return st, idx[: ln.value].copy(), bits(sc[: ln.value]).copy(), float(lq.value)

    # ---- batched forms
    def batch_scan(self, Q):
        torch = self.torch
        if not self.batch:
            with torch.cuda.stream(self.index.stream):
                assert self.e.batch_open() == SLOTS
            self.batch = True
        self.nb = len(Q)
        self.e.query_scan_batch(Q, 0, self.n)
        torch.cuda.synchronize()
        # the pass on the scan's own records first: slots whose lists the batched fast path could not prove exact come back
        # as -1 whatever records follow (their flags are OR-ed with the records'); they must stay few
        self.e.query_lambda_batch(self.e.knn_local_b, 1)
        self.batch_score(TAU)
        own = self._finish_batch(self.e.hits_local_b, 1)
        self.scan_flagged = {b for b in range(self.nb) if own[b]["st"] == -1}
        assert len(self.scan_flagged) <= self.nb // 4 and all(own[b]["st"] == AS_OK for b in range(self.nb) if b not in self.scan_flagged)
        self.e.query_scan_batch(Q, 0, self.n)
        torch.cuda.synchronize()

    def batch_lambda(self, recs, nranks):
        t = self.up(recs)
        self.e.query_lambda_batch(t, nranks)
        self.torch.cuda.synchronize()

    def batch_score(self, tau=TAU):
        self.e.query_score_batch(tau)
        self.torch.cuda.synchronize()

    def batch_finish(self, hits, nranks):
        """-> per slot dict st / n / ids / sbits / lq."""
        return self._finish_batch(self.up(hits), nranks)

    def _finish_batch(self, t, nranks):
        w = max(self.topk, 1)
        idx, sc = np.full((SLOTS, w), -7, dtype=np.int64), np.full((SLOTS, w), np.nan)
        ln, lq, st = np.full(SLOTS, -7, dtype=np.int64), np.full(SLOTS, -7.0), np.full(SLOTS, -7, dtype=np.int32)
        rc = self.L.as_query_finish_batch(self.e.qb, C.c_void_p(t.data_ptr()), nranks, *[a.ctypes.data_as(C.c_void_p) for a in (idx, sc, ln, lq, st)])
        self.torch.cuda.synchronize()
        self.keep.clear()
        assert rc == AS_OK
        assert (st[self.nb:] == -7).all() and (ln[self.nb:] == -7).all()        # idle slots are not reported
        return [dict(st=int(st[b]), n=int(ln[b]), ids=idx[b, : max(ln[b], 0)].copy(), sbits=bits(sc[b, : max(ln[b], 0)]).copy(), lq=float(lq[b]))
                for b in range(self.nb)]

    def close(self):
        self.torch.cuda.synchronize()
        self.index.close()


_OPEN = {}


def steps(name):
    if name not in _OPEN:
        _OPEN[name] = Steps(name)
    return _OPEN[name]


@pytest.fixture(scope="module", autouse=True)
def _indexes():
    yield
    for s in _OPEN.values():
        s.close()
    _OPEN.clear()
    print("\nstaged records: largest |lambda_q - oracle| / oracle per (metric, kernel):",
          {k: float("%.3g" % v) for k, v in sorted(STATS["dev"].items())}, "; bit-exact comparisons (values):", STATS["exact"])


def check_lambda(s, fin, want):
    assert fin["st"] == AS_OK and want >= 1e-3
    dev = abs(fin["lq"] - want) / want
    key = (s.gp["metric"], s.gp["kernel"])
    STATS["dev"][key] = max(STATS["dev"].get(key, 0.0), dev)
    assert dev <= RTOL, (fin["lq"], want, dev)


def check_zero(st, fin):
    """A zero lambda: the step itself reports nothing, the finish returns AS_EZEROLAMBDA, no hit, lambda_q == 0 -- although
    the hit records it was handed are valid."""
    exact([st, fin["st"], fin["n"]], [AS_OK, AS_EZEROLAMBDA, 0])
    exact(bits(fin["lq"]), bits(0.0))


def check_hits(fin, hits, topk):
    want, fl = oracle_np.staged_merge(hits, topk)
    exact(fin["st"], AS_OK)
    exact(fin["n"], len(want))
    exact(fin["ids"], np.array([i for i, _ in want], dtype=np.int64))
    exact(fin["sbits"], bits([x for _, x in want]))
    if "ki" in fin:
        exact([fin["ki"], fin["si"]], list(flags_expected(fl)))
    return want, fl


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", list(CONFIGS))
def test_baseline_own_records_give_clean_flags_and_as_search_answer(name):
    """Before anything hand-built: the scan's own records through the same calls."""
    s = steps(name)
    rng = _rng("baseline", name)
    for _ in range(2):
        q = s.X[rng.integers(0, s.n)] + 0.02 * rng.standard_normal(s.d) / np.sqrt(s.d)
        s.scan(q)
        fin = s.scan_fin
        st, ids, sb, lq = s.as_search(q, TAU)
        exact([fin["st"], fin["ki"], fin["si"], st], [AS_OK, 0, 0, AS_OK])
        exact(fin["ids"], ids)
        exact(fin["sbits"], sb)
        exact(bits(fin["lq"]), bits(lq))
        assert fin["n"] == s.topk and fin["lq"] > 0.0


@pytest.mark.parametrize("name", LAMBDA_CONFIGS)
def test_lambda_step_on_hand_built_records(name):
    """Every single-form case of the config against staged_lambda; the same records with the rank blocks and the slots
    inside them permuted give the same bits (the summation order is the (key, id) rank: fixed by the data alone)."""
    s = steps(name)
    q = case_query(name)
    s.scan(q)
    nq = float(q @ q)
    rng = _rng("perm", name)
    for c in lambda_cases(name):
        st, fin = s.lambda_of(c["recs"], c["m"])
        want, kept = oracle_np.staged_lambda(s.prm, s.tau0, nq, c["recs"][: c["m"]], s.k)
        print(name, c["name"], "m", c["m"], "kept", len(kept), "lambda_q", fin["lq"], "oracle", want)
        if c["zero"]:
            assert want == 0.0
            check_zero(st, fin)
            continue
        exact(st, AS_OK)
        check_lambda(s, fin, want)
        check_hits(fin, s.good_hits, s.topk)          # ... and the finish behind it merges as ever
        st2, fin2 = s.lambda_of(permuted_blocks(c["recs"], s.k, rng))
        exact(st2, AS_OK)
        exact(bits(fin2["lq"]), bits(fin["lq"]))
        if c["tie"]:          # the wrong candidate would have shown: its lambda is far outside the bar
            other = oracle_np.staged_lambda(s.prm, s.tau0, nq, wrong_pick(c["recs"], s.k), s.k)[0]
            assert abs(other - want) >= 1e-6 * want and abs(fin["lq"] - other) >= 0.5e-6 * want


def test_lambda_step_capacity():
    """1 024 records pass (k = 64: capacity_1024 above); 1 025 are refused before anything is launched: the next finish still
    reports the previous lambda_q."""
    s = steps("k64")
    q = case_query("k64")
    s.scan(q)
    c = [c for c in lambda_cases("k64") if c["name"] == "capacity_1024"][0]
    assert c["m"] == REC_CAP == s.L.as_record_capacity(0)
    st, fin = s.lambda_of(c["recs"])
    exact([st, fin["st"]], [AS_OK, AS_OK])
    near = q.copy()
    near[0] += 1.0 / 256.0
    more = np.concatenate([to_records(s.prm, q, near, [7], [0.4]), c["recs"]])     # one record nearer than all the others
    assert len(more) == REC_CAP + 1 and 7 not in oracle_np.rec_ids(c["recs"]) and ranked(more)[0] == 0
    exact(s.lam(more), AS_EUNSUPPORTED)
    fin2 = s.finish(s.good_hits)
    exact(fin2["st"], AS_OK)
    exact(bits(fin2["lq"]), bits(fin["lq"]))
    assert oracle_np.staged_lambda(s.prm, s.tau0, float(q @ q), more, s.k)[0] != oracle_np.staged_lambda(s.prm, s.tau0, float(q @ q), c["recs"], s.k)[0]


@pytest.mark.parametrize("name,R", [("k5", 2), ("k5", 8), ("k63", 2), ("k65", 8), ("k120", 2), ("k120", 8), ("k120c", 8)])
def test_lambda_of_real_records_does_not_depend_on_their_layout(name, R):
    """The scan's own k records of a whole-space scan, scattered over R rank blocks in a random permutation with -1
    padding: lambda_q equals, bit for bit, that of the unpermuted block and as_search's."""
    s = steps(name)
    rng = _rng("real", name, R)
    for _ in range(3):
        q = s.X[rng.integers(0, s.n)] + 0.02 * rng.standard_normal(s.d) / np.sqrt(s.d)
        s.scan(q)
        own = s.e.knn_local.cpu().numpy().copy()
        fin = s.scan_fin
        valid = own[oracle_np.rec_ids(own) >= 0]
        assert len(valid) >= 1
        st, fin2 = s.lambda_of(scatter(valid, R, s.k, rng))
        lq = s.as_search(q, TAU)[3]
        exact([st, fin2["st"]], [AS_OK, AS_OK])
        exact(bits([fin2["lq"], lq]), bits([fin["lq"], fin["lq"]]))
        check_lambda(s, fin, oracle_np.staged_lambda(s.prm, s.tau0, float(s.q @ s.q), own, s.k)[0])


def test_lambda_step_is_a_no_op_under_feature_lambda():
    """Feature mode: lambda_q comes from the scan; garbage records leave it untouched."""
    from conftest import calibrate_feature_eps
    s = Steps("k5", extra={"lambda_mode": "feature", "eps": calibrate_feature_eps(config_data("k5")[0], 5, "cosine")})
    try:
        q = case_query("k5")
        s.scan(q)
        fin = s.scan_fin
        assert fin["st"] == AS_OK and fin["lq"] > 0.0
        s.scan_only(q)
        garbage = empties(3 * s.k)
        garbage[::2, 0] = id_bits(np.arange(len(garbage[::2])))
        exact(s.lam(garbage), AS_OK)
        exact(s.lam(np.zeros((REC_CAP + 1, 6))), AS_EUNSUPPORTED)     # (the capacity check comes first, as in item mode)
        s.score(TAU)
        fin2 = s.finish()
        exact([fin2["st"], fin2["ki"], fin2["si"]], [AS_OK, 0, 0])
        exact(bits(fin2["lq"]), bits(fin["lq"]))
        exact(fin2["ids"], fin["ids"])
        exact(fin2["sbits"], fin["sbits"])
    finally:
        s.close()


@pytest.mark.parametrize("name,nranks", [("k5", 1), ("k5", 3), ("k5", 8), ("k65", 3), ("k120", 8), ("k120c", 3)])
def test_batched_lambda_step(name, nranks):
    """[rank][slot][k]: every slot against staged_lambda, and bit-equal to the single form on the slot's records
    flattened in rank order."""
    s = steps(name)
    Q, recs, flat, counts = batch_lambda_case(name, nranks)
    assert s.k * nranks <= REC_CAP
    s.batch_scan(Q)
    s.batch_lambda(recs, nranks)
    s.batch_score(TAU)
    per = s.topk + 1
    hits = hit_case("plain", s.topk, nranks * per, nranks, _rng("bl-hits", name, nranks), flags=(0,) * (nranks - 1)).reshape(nranks, 1, per, 2)
    hits = np.ascontiguousarray(np.repeat(hits, SLOTS, axis=1))
    got = s.batch_finish(hits, nranks)
    nzero = 0
    for b in range(len(Q)):
        want, kept = oracle_np.staged_lambda(s.prm, s.tau0, float(Q[b] @ Q[b]), flat[b], s.k)
        exact(len(kept), min(counts[b], s.k))
        if b in s.scan_flagged:
            exact([got[b]["st"], got[b]["n"]], [-1, 0])
            continue
        s.scan(Q[b])
        st, one = s.lambda_of(flat[b])
        exact([st, one["st"]], [AS_OK, got[b]["st"]])
        exact(bits(one["lq"]), bits(got[b]["lq"]))
        if want == 0.0:
            exact([got[b]["st"], got[b]["n"]], [AS_EZEROLAMBDA, 0])
            exact(bits(got[b]["lq"]), bits(0.0))
            nzero += 1
        else:
            check_lambda(s, got[b], want)
            check_hits(got[b], hits[:, b].reshape(-1, 2), s.topk)
    assert nzero >= 1


HIT_CONFIGS = [("k7p", 1), ("k5", 15), ("k64", 64), ("cap", 1024)]


@pytest.mark.parametrize("R", [1, 2, 8])
@pytest.mark.parametrize("name,topk", HIT_CONFIGS)
def test_hit_merge_on_hand_built_records(name, topk, R):
    """m = R (topk + 1) records of every kind against staged_merge: ids, score bits, length, flags; permuting the rank blocks
    and the records inside a block leaves the answer identical."""
    s = steps(name)
    assert s.topk == topk
    s.scan(case_query(name))
    rng = _rng("hits", name, R)
    m = R * (topk + 1)
    for kind in HIT_KINDS:
        hits = hit_case(kind, topk, m, R, rng, flags=(0,) * (R - 1))
        fin = s.finish(hits)
        want, fl = check_hits(fin, hits, topk)
        assert fl == 0 and fin["lq"] > 0.0
        print(name, "R", R, kind, "m", m, "returned", fin["n"])
        fin2 = s.finish(permuted_blocks(hits, topk + 1, rng))
        for f in ("st", "n", "ids", "sbits", "ki", "si"):
            exact(fin2[f], fin[f])
        if kind == "fewer_than_topk":
            assert fin["n"] == topk // 2 < topk
        if kind in ("tie_at_the_cut", "tie_run_across_the_cut"):
            ids, sc = oracle_np.rec_ids(hits), hits[:, 1]
            left_out = [i for i in np.nonzero(ids >= 0)[0] if sc[i] == want[-1][1] and ids[i] not in set(fin["ids"].tolist())]
            assert left_out and all(ids[i] > want[-1][0] for i in left_out)        # the tie at the cut went to the lower id
        if kind == "all_scores_equal":
            assert fin["ids"].tolist() == sorted(oracle_np.rec_ids(hits)[oracle_np.rec_ids(hits) >= 0].tolist())[:topk]
        if kind == "minus_inf_valid":
            assert fin["n"] == topk             # the -inf records are valid: they rank last, ahead of the +inf / NaN empties
            assert np.isneginf(fin["sbits"].view(np.float64)).any()


def test_hit_merge_capacity():
    """8 208 records pass, 8 209 are refused; the workspace still answers afterwards."""
    s = steps("cap")
    s.scan(case_query("cap"))
    assert s.L.as_record_capacity(1) == HIT_CAP == 8 * (s.topk + 1) + 8
    rng = _rng("hitcap")
    hits = hit_case("tie_run_across_the_cut", s.topk, HIT_CAP, 8, rng, flags=(0,) * 8)
    fin = s.finish(hits)
    check_hits(fin, hits, s.topk)
    assert fin["n"] == s.topk
    more = np.concatenate([hits, hit_case("plain", s.topk, 1, 1, rng)])
    bad = s.finish(more)
    exact([bad["st"], bad["n"]], [AS_EUNSUPPORTED, -7])
    again = s.finish(hits)
    for f in ("st", "n", "ids", "sbits"):
        exact(again[f], fin[f])


@pytest.mark.parametrize("name,R", [("k5", 3), ("cap", 8)])
def test_flag_records(name, R):
    """Each bit alone in a non-first rank's block, several records OR-ed, none at all: as_query_flags reports bit 1 / 2 as
    bit 0 of knn_inexact / score_inexact and bit 4 / 8 as their bit 1 (16 and 32 are the one-exchange pass's and the
    failed-rank bit: not part of as_query_flags); the answer itself is merged all the same."""
    s = steps(name)
    s.scan(case_query(name))
    rng = _rng("flags", name)
    m = R * (s.topk + 1)
    for flags in [(1,), (2,), (4,), (8,), (16,), (32,), (1, 8), (2, 4, 0), (1, 2, 4, 8), (4, 4), ()]:
        hits = hit_case("plain", s.topk, m, R, rng, flags=flags)
        ids = oracle_np.rec_ids(hits)
        assert (ids == -2).sum() == len(flags) and (ids[: s.topk + 1] != -2).all()
        fin = s.finish(hits)
        want, fl = check_hits(fin, hits, s.topk)
        exact(fl, int(np.bitwise_or.reduce(np.array(flags + (0,)))))
    fin = s.finish(hit_case("plain", s.topk, m, R, rng, flags=(0,) * R))
    exact([fin["ki"], fin["si"]], [0, 0])              # ... and nothing sticks to the workspace


@pytest.mark.parametrize("name,nranks", [("k5", 1), ("k5", 3), ("k5", 8), ("cap", 8)])
def test_batched_hit_merge(name, nranks):
    """[rank][slot][topk + 1]: per-slot kinds as above; a slot with a flag bit comes back as -1 (rerun) with no hit, a slot
    whose lambda step said zero as AS_EZEROLAMBDA."""
    s = steps(name)
    nb = 13 if name == "cap" else 29
    rng = _rng("bhits", name, nranks)
    Q = np.stack([case_query(name, row=b) for b in range(nb)])
    recs = np.empty((nranks, SLOTS, s.k, 6))
    zero_slot, flag_slots = 5, {2: 8, 3: 4, 7: 1, 9: 2, 11: 32, 12: 16}          # every bit, one slot each
    for b in range(SLOTS):
        nv = 0 if b == zero_slot or b >= nb else s.k + 2
        recs[:, b] = scatter(make_valid(s.prm, Q[min(b, nb - 1)], rng, min(nv, nranks * s.k), s.k)[0], nranks, s.k, rng).reshape(nranks, s.k, 6)
    per = s.topk + 1
    hits = np.empty((nranks, SLOTS, per, 2))
    for b in range(SLOTS):
        fl = (flag_slots[b],) if b in flag_slots else ((0,) * (nranks - 1) if b % 2 else ())
        hits[:, b] = hit_case(HIT_KINDS[b % len(HIT_KINDS)], s.topk, nranks * per, nranks, rng, flags=fl).reshape(nranks, per, 2)
    s.batch_scan(Q)
    s.batch_lambda(recs, nranks)
    s.batch_score(TAU)
    got = s.batch_finish(hits, nranks)
    for b in range(nb):
        flat = hits[:, b].reshape(-1, 2)
        want, fl = oracle_np.staged_merge(flat, s.topk)
        if b in s.scan_flagged:
            exact([got[b]["st"], got[b]["n"]], [-1, 0])
        elif b in flag_slots:
            exact([fl, got[b]["st"], got[b]["n"]], [flag_slots[b], -1, 0])
        elif b == zero_slot:
            exact([got[b]["st"], got[b]["n"]], [AS_EZEROLAMBDA, 0])
            exact(bits(got[b]["lq"]), bits(0.0))
        else:
            assert fl == 0 and got[b]["lq"] > 0.0
            check_hits(got[b], flat, s.topk)
