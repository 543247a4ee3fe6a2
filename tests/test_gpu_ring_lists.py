"""GPU: the ring's per-row bookkeeping between the block passes -- knn_fold_kernel, knn_merge_kernel and
knn_thresholds_kernel through as_knn_fold / as_knn_merge / as_knn_thresholds -- on hand-built slices, against the numpy
model in oracle/oracle_np.py (ring_fold, ring_merge, ring_thresholds), bit for bit.

The space holds items with entries in {0, +-0.5, +-1, +-2} (d = 8): squared norms are small dyadic numbers that differ
from a row to the four rows before it, so a wrong row offset changes the answer.  as_ring_i8_set(sp, 0, 2^-6, 1) fixes the
error coefficient at 2^-12 + 12 * 2^-24: its product with a sum of two such norms is exact in fp64, fused
or not, so bounds can be put exactly on a proof's edge or one fp32 ulp to either side of it and every expected bound, flag
and threshold is compared as bits.  The entries (keys, dist, gy, ids) are arbitrary numbers: the kernels only move them.
Slots past a slice's count hold NaN / -7 on the way in and are not looked at on the way out.

The generators need no GPU: tests/test_ring_lists_inputs.py checks on the CPU that the model agrees with a sorted()
restatement on them, that every "edge +- 1 ulp" input lies on the side its name says (Fraction arithmetic), that the
exact-coefficient products are exact, and that the soundness inputs flag 20 - 80 % of their rows."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle_np

pytestmark = pytest.mark.gpu

D = 8
SPACE_N = 1031
ROW_SIZES = [1, 3, 4, 5, 1027]                 # 1027: 256 launch blocks of four waves and a tail of three rows
WIDTHS = [(32, 5), (64, 25), (128, 120)]       # (M, k) with M = as_knn_list_width(k)
COEF = 2.0 ** -12 + 12 * 2.0 ** -24            # as_ring_i8_set(sp, 0.0, 2^-6, 1)
DP = 32                                        # d = 8 pads to 32 columns
EPS = {"l2": 1.5, "cosine": 0.75}
POISON_ID = -7
SENTINEL = -123.0
F32_INF = np.float32(np.inf)
AS_EINVAL, AS_EUNSUPPORTED = 1, 4


def _metric(metric):
    return oracle_np.METRIC_L2 if metric == "l2" else oracle_np.METRIC_COSINE


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------ the space
@functools.lru_cache(maxsize=None)
def space_items():
    """-> (X [SPACE_N][8], squared norms).  Row 5 is the zero item; every other norm is positive and differs from the
    norms of the four rows before it."""
    rng = np.random.default_rng(2024)
    values = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    X, n = np.zeros((SPACE_N, D)), []
    for i in range(SPACE_N):
        while True:
            x = np.zeros(D) if i == 5 else values[rng.integers(0, len(values), D)]
            s = float(x @ x)
            if i == 5 or (s > 0 and all(s != n[j] for j in range(max(0, i - 4), i))):
                break
        X[i] = x
        n.append(s)
    return _ro(X, np.array(n))


def empty_slice(rows, M):
    """A slice without an entry: count 0, no dropped bit, bound +inf; every slot poisoned."""
    return (np.full((rows, M), np.nan), np.full((rows, M), np.nan), np.full((rows, M), np.nan),
            np.full((rows, M), POISON_ID, dtype=np.int32), np.zeros(rows, dtype=np.int32), np.full(rows, np.inf, dtype=np.float32))


def _entries(rng, count, ids, nkeys=24):
    """`count` entries on `ids` (distinct): keys from a pool of nkeys multiples of 1/8 (ties are the rule), dist and gy
    numbers that identify their entry; ordered by (key, id)."""
    key = rng.integers(0, nkeys, count) / 8.0
    o = np.lexsort((ids, key))
    key, ids = key[o], ids[o]
    return key, 0.5 * key + (ids % 1000) * 1e-3, -key + (ids % 777), ids


def _put(sl, r, key, dist, gy, idx):
    c = len(key)
    sl[0][r, :c], sl[1][r, :c], sl[2][r, :c], sl[3][r, :c] = key, dist, gy, idx


def _row_ids(rng, r, M, count):
    """Distinct int32 ids of one row: a global offset on even rows, the last ids below 2^31 on odd ones."""
    base = 2 ** 31 - 4 * M if r % 2 else 100000
    return (base + rng.choice(4 * M, size=count, replace=False)).astype(np.int32)


# ------------------------------------------------------------------------------------------------ fold inputs
BOUND_KINDS = ["run_below", "run_above", "run_equal", "blk_pinf", "blk_ninf", "run_pinf"]


def fold_patterns(M):
    """(c_run, c_blk), (dropped_run, dropped_blk), bound kind: counts 0 + 0, 0 + c, c + 0, M + M, C = M - 1, M, M + 1 and
    a few more; every combination of the two bits (a block slice 0 | 1 << 30 included); the running bound one fp32 ulp
    below / above / on the block's new bound, block bounds of +-inf, a running bound of +inf."""
    c = M // 3
    counts = [(0, 0), (0, c), (c, 0), (M, M), (c, M - 1 - c), (M - c, c), (c + 1, M - c), (M, 0), (0, M), (1, M)]
    bits = [(0, 0), (0, 1), (1, 0), (1, 1)]
    return [(cc, bb, bd) for cc in counts for bb in bits for bd in BOUND_KINDS]


def _block_bound(rng):
    """An fp32 bound in one of six binades (the rounding of bound - e falls differently in each)."""
    return np.float32(float(rng.choice([1.5, 3.25, 5.0, 9.75, 21.5, 40.0])) + int(rng.integers(0, 4096)) * 2.0 ** -12)


@functools.lru_cache(maxsize=None)
def fold_case(M, metric, rows, row_begin, mode, seed=0):
    """-> dict(run, blk, flag, nmax_b, n_rows, kinds): one fold's inputs, row r made after pattern (r + seed) of a
    shuffled fold_patterns(M)."""
    rng = np.random.default_rng(1000 * M + 10 * rows + row_begin + 100 * mode + seed + (7 if metric == "cosine" else 0))
    pats = fold_patterns(M)
    pats = [pats[i] for i in rng.permutation(len(pats))]
    n_rows = space_items()[1][row_begin : row_begin + rows]
    nmax_b = float(rng.choice([2.75, 9.5, 33.0]))
    run, blk = empty_slice(rows, M), empty_slice(rows, M)
    kinds = []
    for r in range(rows):
        (c_run, c_blk), (d_run, d_blk), kind = pats[(r + seed) % len(pats)]
        ids = _row_ids(rng, r, M, c_run + c_blk)
        _put(run, r, *_entries(rng, c_run, ids[:c_run]))
        _put(blk, r, *_entries(rng, c_blk, ids[c_run:]))
        run[4][r], blk[4][r] = c_run | (d_run << 30), c_blk | (d_blk << 30)
        bt = _block_bound(rng)
        if kind == "blk_pinf":
            bt = F32_INF
        elif kind == "blk_ninf":
            bt = -F32_INF
        nb = oracle_np.rd32(float(bt) - oracle_np.ring_err(COEF, _metric(metric), float(n_rows[r]), nmax_b))
        if kind == "run_below":
            rt = np.nextafter(nb, -F32_INF)
        elif kind == "run_above":
            rt = np.nextafter(nb, F32_INF)
        elif kind == "run_equal":
            rt = nb
        elif kind == "run_pinf":
            rt = F32_INF
        else:
            rt = _block_bound(rng)
        run[5][r], blk[5][r] = rt, bt          # (a bound is stored whatever the bit says: without the bit it must not count)
        kinds.append(kind)
    flag = np.where(rng.random(rows) < 0.45, rng.integers(1, 4, rows), 0).astype(np.int32)
    if mode and rows > 1:
        flag[(rows // 2 + 1) % rows], flag[rows // 2] = 0, 2
    return dict(run=_ro(*run), blk=_ro(*blk), flag=_ro(flag)[0], nmax_b=nmax_b, n_rows=n_rows, kinds=kinds)


def fold_expected(case, M, metric, mode, coef=COEF):
    return oracle_np.ring_fold(case["run"], case["blk"], M, _metric(metric), coef, case["n_rows"], case["nmax_b"], mode, case["flag"])


FOLD_CONFIGS = [(rows, 0, 0) for rows in ROW_SIZES] + [(1027, 3, 0), (1027, 0, 1), (1027, 3, 2), (5, 3, 1), (4, 0, 2)]   # (rows, row_begin, mode)


@functools.lru_cache(maxsize=None)
def chain_case(M, metric, rows=261, row_begin=3):
    """Five block slices for a running list that starts empty; then the second round's two folds (mode 2, mode 1) on a
    scattered set of rows.  -> (blocks, nmax, modes, flag, n_rows)"""
    rng = np.random.default_rng(77 + M + (1 if metric == "cosine" else 0))
    n_rows = space_items()[1][row_begin : row_begin + rows]
    blocks, nmax = [], []
    for b in range(7):
        sl = empty_slice(rows, M)
        for r in range(rows):
            c = int(rng.choice([0, 1, M // 4, M // 2, M - 1, M]))
            ids = (b * 4 * M + _row_ids(rng, r, M, c).astype(np.int64) - (7 * 4 * M if r % 2 else 0)).astype(np.int32)
            _put(sl, r, *_entries(rng, c, ids))
            sl[4][r] = c | (int(rng.integers(0, 2)) << 30)
            sl[5][r] = rng.choice([_block_bound(rng), F32_INF, -F32_INF], p=[0.8, 0.1, 0.1])
        blocks.append(_ro(*sl))
        nmax.append(float(rng.choice([2.75, 9.5, 33.0])))
    flag = np.where(rng.random(rows) < 0.4, 1, 0).astype(np.int32)
    return blocks, nmax, [0, 0, 0, 0, 0, 2, 1], _ro(flag)[0], n_rows


def chain_expected(M, metric):
    blocks, nmax, modes, flag, n_rows = chain_case(M, metric)
    run, out = empty_slice(len(flag), M), []
    for sl, nm, mode in zip(blocks, nmax, modes):
        run = oracle_np.ring_fold(run, sl, M, _metric(metric), COEF, n_rows, nm, mode, flag)
        out.append(run)
    return out


def default_coef_case(metric, rows=96, row_begin=3, M=32):
    """The block's bound alone decides (empty running list, dropped bit set), under the space's default coefficient."""
    rng = np.random.default_rng(5 + (1 if metric == "cosine" else 0))
    n_rows = space_items()[1][row_begin : row_begin + rows]
    run, blk = empty_slice(rows, M), empty_slice(rows, M)
    for r in range(rows):
        blk[4][r] = 1 << 30
        blk[5][r] = _block_bound(rng)
    return dict(run=run, blk=blk, flag=np.zeros(rows, dtype=np.int32), nmax_b=9.5, n_rows=n_rows, row_begin=row_begin, M=M)


def f32_floor(q):
    """The largest fp32 not above the rational q."""
    f = np.float32(float(q))
    while Fraction(float(f)) > q:
        f = np.nextafter(f, -F32_INF)
    while Fraction(float(np.nextafter(f, F32_INF))) <= q:
        f = np.nextafter(f, F32_INF)
    return f


# ------------------------------------------------------------------------------------------------ merge inputs
PROOF_KINDS = ["none", "edge_equal", "edge_above", "edge_below", "far_above", "pos_inf", "neg_inf", "nan",
               "zero_entry_unproven", "zero_entry_proven"]
EXPECT_FLAG = dict(none=0, edge_equal=1, edge_above=0, edge_below=1, far_above=0, pos_inf=0, neg_inf=1, nan=1, far_below=1,
                   zero_entry_unproven=1, zero_entry_proven=0)
MERGE_KINDS = [(npk, proof, tie) for npk in ("lt", "eq", "gt") for proof in PROOF_KINDS for tie in (False, True)]
MERGE_ROWS = 123          # two rows of every kind and a tail; 31 launch blocks


@functools.lru_cache(maxsize=None)
def merge_case(M, k, metric, nblocks, row_begin, seed=0):
    """nblocks >= 1: that many slices and their block_nmax; 0: one folded slice (e_b = 0).  Row r is made after
    MERGE_KINDS[(r + seed) % 60] = (passing entries < k / = k / > k, the proof, "the k-th and (k+1)-th key tie"):
      none            no slice carries the dropped bit (their bounds are -inf or NaN and must not count)
      edge_*          one slice's bound minus its error term sits ON B / one fp32 ulp above / below it, every other slice
                      with the bit is proven (B = the k-th passing key; rows with fewer passing entries have B = epskey, which
                      no fp32 bound meets exactly: they take far_below / far_above / far_below instead)
      far_above, pos_inf, neg_inf, nan      the deciding slice's bound
      zero_entry_*    the deciding slice holds NO entry and carries the bit
    Among the entries that fail eps: one key an ulp above epskey, a NaN key; rows with more than k passing entries end
    their passing keys ON epskey.
    -> dict(slices, block_nmax (None when folded), n_rows, eps, kinds (the proof kind each row really got), stars (each
    row's deciding slice))"""
    rng = np.random.default_rng(31 * M + 7 * nblocks + row_begin + seed + (3 if metric == "cosine" else 0))
    nsl, folded = max(nblocks, 1), nblocks == 0
    rows, m = MERGE_ROWS, _metric(metric)
    eps = EPS[metric]
    ek = eps * eps if metric == "l2" else eps
    n_rows = space_items()[1][row_begin : row_begin + rows]
    block_nmax = None if folded else [float(v) for v in rng.choice([0.25, 2.75, 9.5, 33.0], nsl)]
    slices = [empty_slice(rows, M) for _ in range(nsl)]
    pool = np.arange(0, int(ek * 32)) / 32.0           # passing keys strictly below epskey
    kinds, stars = [], []
    for r in range(rows):
        npk, proof, tie = MERGE_KINDS[(r + seed) % len(MERGE_KINDS)]
        star = int(rng.integers(0, nsl))               # the deciding slice
        zero = proof.startswith("zero_entry")
        room = (nsl - 1 if zero else nsl) * M
        npass = min(room, {"lt": int(rng.integers(0, k)), "eq": k, "gt": k + int(rng.integers(1, 2 * k + 1))}[npk])
        nfail = int(min(room - npass, rng.integers(0, 6)))
        key = np.sort(rng.choice(pool, npass))
        if npass > k and tie:
            key[k] = key[k - 1]
            key = np.sort(key)
        if npass > k + 1:
            key[-1] = ek                               # exactly on eps: passes
        e = [0.0 if folded else oracle_np.ring_err(COEF, m, float(n_rows[r]), block_nmax[b]) for b in range(nsl)]
        if npass >= k:
            v = key[k - 1]
            t = np.float32(v + e[star])
            B = float(t) - e[star]                     # the k-th key, moved by less than an fp32 ulp onto bound - e
            key[key == v] = B
        else:
            B, t = ek, None
            proof = {"edge_equal": "far_below", "edge_above": "far_above", "edge_below": "far_below"}.get(proof, proof)
        fail = np.array([np.nextafter(ek, np.inf), np.nan, ek + 0.5, 4.0 * ek, np.nan, ek + 1.0])[:nfail]
        key = np.concatenate([key, fail])
        ids = _row_ids(rng, r, max(M, (len(key) + 3) // 4), len(key))
        dist, gy = 0.5 * key + (ids % 1000) * 1e-3, -key + (ids % 777)
        # deal the entries to the slices (none to a zero-entry deciding slice), M at the most each
        slots = np.repeat([b for b in range(nsl) if not (zero and b == star)], M)
        owner = rng.permutation(slots)[: len(key)]
        far = lambda b: np.float32(B + e[b] + 0.5)
        for b in range(nsl):
            sel = np.nonzero(owner == b)[0]
            kb = np.where(np.isnan(key[sel]), np.inf, key[sel])
            sel = sel[np.lexsort((ids[sel], kb))]      # (key, id); a NaN key at the end
            _put(slices[b], r, key[sel], dist[sel], gy[sel], ids[sel])
            bit = 0 if proof == "none" else int(rng.integers(0, 2))
            slices[b][4][r] = len(sel) | (bit << 30)
            slices[b][5][r] = far(b) if bit else rng.choice([-F32_INF, np.float32(np.nan)])
        if proof != "none":
            slices[star][4][r] |= 1 << 30
            slices[star][5][r] = {"edge_equal": t, "edge_above": None if t is None else np.nextafter(t, F32_INF),
                                  "edge_below": None if t is None else np.nextafter(t, -F32_INF), "far_above": far(star),
                                  "far_below": np.float32(B + e[star] - 0.5), "pos_inf": F32_INF, "neg_inf": -F32_INF,
                                  "nan": np.float32(np.nan), "zero_entry_unproven": np.float32(B + e[star] - 0.5),
                                  "zero_entry_proven": far(star)}[proof]
        kinds.append(proof)
        stars.append(star)
    return dict(slices=[_ro(*s) for s in slices], block_nmax=block_nmax, n_rows=n_rows, eps=eps, kinds=kinds, stars=stars)


def merge_expected(case, M, k, metric):
    return oracle_np.ring_merge(case["slices"], M, k, _metric(metric), COEF, case["eps"], case["n_rows"], case["block_nmax"])


# (M, k, nblocks, row_begin): 18 blocks of width 128 are the most the merge kernel's LDS takes
MERGE_CONFIGS = [(128, 120, 0, 0), (128, 120, 1, 3), (128, 120, 2, 0), (128, 120, 5, 3), (128, 120, 18, 3),
                 (32, 5, 0, 3), (32, 5, 5, 0), (64, 25, 0, 0), (64, 25, 5, 3)]


# ------------------------------------------------------------------------------------------------ threshold inputs
THRESHOLD_ROWS = [1, 255, 256, 257]


@functools.lru_cache(maxsize=None)
def thresholds_case(M, rows, row_begin):
    """cnt = M - 1 (the M-th slot poisoned), M and M | 1 << 30 in turn; M-th keys in several binades."""
    rng = np.random.default_rng(9 * M + rows + row_begin)
    key = np.sort(rng.choice([0.37, 1.1, 2.9, 7.3], (rows, 1)) * rng.random((rows, M)), axis=1)
    cnt = np.array([(M - 1, M, M | (1 << 30))[(r + row_begin) % 3] for r in range(rows)], dtype=np.int32)
    key[(cnt & 0xFFFF) < M, M - 1] = np.nan
    return _ro(key, cnt) + (space_items()[1][row_begin : row_begin + rows],)


# ------------------------------------------------------------------------------------------------ soundness inputs
SOUND_N, SOUND_K, SOUND_M = 600, 24, 32                     # k above M / 4: a slice cut at 8 entries can hide a neighbour
SOUND_CUTS = [0, 40, 240, 370, 399, 600]
SOUND_EPS = {"l2": 3.5, "cosine": 0.5}
SOUND_WIDTH_P = [0.5, 0.25, 0.25]                           # how often a slice keeps M / 4, M / 2, M entries


@functools.lru_cache(maxsize=None)
def soundness_case(metric):
    """600 items (entries multiples of 1/8: the norms and the coefficient's products stay exact) in 5 uneven column
    blocks; every row against every block by brute force in fp64.  A block's slice keeps its M' smallest entries, M' from
    {8, 16, 32} per row and block (8 half of the time); where that cut something, the dropped bit and t32 = the smallest dropped key rounded
    down to fp32 (truthful: a lower bound of everything dropped).
    -> dict(X, n64, slices, block_nmax, eps, brute = (idx, key, cnt) of the k nearest inside eps by (key, id))"""
    rng = np.random.default_rng(99)
    X = rng.integers(-16, 17, (SOUND_N, D)) / 8.0
    n64 = np.einsum("ij,ij->i", X, X)
    m, k, M = _metric(metric), SOUND_K, SOUND_M
    eps = SOUND_EPS[metric]
    ek = eps * eps if metric == "l2" else eps
    nb = len(SOUND_CUTS) - 1
    slices = [empty_slice(SOUND_N, M) for _ in range(nb)]
    b_idx, b_key, b_cnt = np.full((SOUND_N, k), -1, dtype=np.int32), np.zeros((SOUND_N, k)), np.zeros(SOUND_N, dtype=np.int32)
    for i in range(SOUND_N):
        key, dist, gy = oracle_np.pair_quantities(X[i], X, n64[i], n64, m)
        ids = np.arange(SOUND_N)
        o = np.lexsort((ids, key))
        o = o[o != i]
        best = o[key[o] <= ek][:k]
        b_idx[i, : len(best)], b_key[i, : len(best)], b_cnt[i] = best, key[best], len(best)
        for b in range(nb):
            ob = o[(o >= SOUND_CUTS[b]) & (o < SOUND_CUTS[b + 1])]
            keep = int(rng.choice([M // 4, M // 2, M], p=SOUND_WIDTH_P))
            kept, cut = ob[:keep], ob[keep:]
            _put(slices[b], i, key[kept], dist[kept], gy[kept], kept.astype(np.int32))
            slices[b][4][i] = len(kept) | ((1 << 30) if len(cut) else 0)
            slices[b][5][i] = oracle_np.rd32(float(key[cut[0]])) if len(cut) else F32_INF
    block_nmax = [float(n64[SOUND_CUTS[b] : SOUND_CUTS[b + 1]].max()) for b in range(nb)]
    return dict(X=_ro(X)[0], n64=n64, slices=[_ro(*s) for s in slices], block_nmax=block_nmax, eps=eps, brute=(b_idx, b_key, b_cnt))


def soundness_expected(metric):
    """-> (the folded slice, the merge of it, the merge of the five slices) by the model."""
    c = soundness_case(metric)
    m, run = _metric(metric), empty_slice(SOUND_N, SOUND_M)
    for sl, nm in zip(c["slices"], c["block_nmax"]):
        run = oracle_np.ring_fold(run, sl, SOUND_M, m, COEF, c["n64"], nm)
    return (run, oracle_np.ring_merge([run], SOUND_M, SOUND_K, m, COEF, c["eps"], c["n64"]),
            oracle_np.ring_merge(c["slices"], SOUND_M, SOUND_K, m, COEF, c["eps"], c["n64"], c["block_nmax"]))


# ------------------------------------------------------------------------------------------------ GPU side
# tests/test_ring_lists_inputs.py imports this module on machines without a GPU: nothing above imports torch or
# pyarrowspace_amd or touches a device; the helpers and tests below import them where they run.
GUARD = 2        # rows of sentinels after the rows a call may write


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class _Space:
    """One space per metric (shared by the tests of this file: they only read it) and the raw calls on it."""

    def __init__(self, metric, X, ring=True):
        import torch

        from pyarrowspace_amd import _lib
        from pyarrowspace_amd.dist import HipEngine
        self.torch, self.lib, self.metric = torch, _lib, metric
        self.e = HipEngine({"eps": 1.0, "k": 5, "topk": 5, "p": 2.0, "sigma": None, "metric": metric})
        self.e.create_space(torch.from_numpy(np.array(X)).cuda())        # (a writable copy: the generators' arrays are read-only)
        self.L, self.sp = self.e.L, self.e.sp
        st = self.e.ring_i8_stats()
        assert st[2] == 0.0, st
        self.set_ring(ring)

    def set_ring(self, on):
        """The documented ring switch: the exact coefficient 2^-12 + 12 * 2^-24, or back to the space's default one."""
        got = self.e.ring_i8_set(0.0, 2.0 ** -6, bool(on))
        assert got == bool(on)

    def gp(self, k, eps=1.0):
        return self.lib.GraphParams(eps, k, 5, 2.0, 1.0, 1, 0)

    def dev(self, a, before=0, fill=None):
        """`a` on the device behind `before` rows and in front of GUARD rows of a sentinel -> (tensor, pointer to a's row 0)."""
        a = np.ascontiguousarray(a)
        pad = np.empty((before + a.shape[0] + GUARD,) + a.shape[1:], dtype=a.dtype)
        pad[...] = (SENTINEL if a.dtype.kind == "f" else -99) if fill is None else fill
        pad[before : before + a.shape[0]] = a
        t = self.torch.from_numpy(pad).cuda()
        return t, C.c_void_p(t.data_ptr() + before * t.stride(0) * t.element_size())

    def back(self, t, before, rows):
        """-> (the rows a call owns, True when every row before and after them still holds what dev() put there)."""
        h = t.cpu().numpy()
        own = h[before : before + rows]
        rest = np.concatenate([h[:before], h[before + rows :]])
        ref = np.empty_like(rest)
        ref[...] = SENTINEL if h.dtype.kind == "f" else -99
        return own, bool(np.array_equal(_bits(rest), _bits(ref)))

    def fold(self, k, row_begin, mode, nmax_b, flag, run, blk, expect=0):
        rows = len(run[4])
        r = [self.dev(a, row_begin) for a in run]
        b = [self.dev(a, row_begin) for a in blk]
        f = self.dev(flag, row_begin)
        gp = self.gp(k)
        self.torch.cuda.synchronize()
        st = self.L.as_knn_fold(self.sp, C.byref(gp), row_begin, row_begin + rows, mode, float(nmax_b), f[1] if mode else C.c_void_p(),
                                *[p for _, p in r], *[p for _, p in b])
        assert st == expect, (st, self.lib.last_error())
        out = [self.back(t, row_begin, rows) for t, _ in r]
        assert all(ok for _, ok in out), "as_knn_fold wrote outside its rows"
        for (t, _), a in zip(b, blk):
            assert np.array_equal(_bits(self.back(t, row_begin, rows)[0]), _bits(a)), "as_knn_fold changed the block's slice"
        return tuple(o for o, _ in out)

    def merge(self, k, eps, row_begin, nblocks, slices, block_nmax, expect=0):
        rows = len(slices[0][4])
        torch = self.torch
        p = [torch.from_numpy(np.ascontiguousarray(np.stack([s[j] for s in slices]))).cuda() for j in range(6)]
        outs = [self.dev(np.full(shape, fill, dtype=dt)) for shape, fill, dt in
                (((rows, k), -5, np.int32), ((rows, k), SENTINEL, np.float64), ((rows, k), SENTINEL, np.float64),
                 ((rows, k), SENTINEL, np.float64), ((rows,), -5, np.int32), ((rows,), -5, np.int32), ((rows,), SENTINEL, np.float64))]
        nm = (C.c_double * max(nblocks, 1))(*(block_nmax or [0.0]))
        nf = C.c_int64(-1)
        gp = self.gp(k, eps)
        torch.cuda.synchronize()
        st = self.L.as_knn_merge(self.sp, C.byref(gp), row_begin, row_begin + rows, nblocks, *[C.c_void_p(t.data_ptr()) for t in p],
                                 C.cast(nm, C.c_void_p) if nblocks else C.c_void_p(), *[ptr for _, ptr in outs], C.byref(nf))
        assert st == expect, (st, self.lib.last_error())
        got = [self.back(t, 0, rows) for t, _ in outs]
        assert all(ok for _, ok in got), "as_knn_merge wrote outside its rows"
        names = ("idx", "key", "dist", "gy", "cnt", "flag", "band")
        res = {n: g for n, (g, _) in zip(names, got)}
        res["nflagged"] = int(nf.value)
        return res

    def thresholds(self, k, row_begin, nmax_all, key, cnt, expect=0):
        rows = len(cnt)
        kd, cd = self.dev(key, row_begin), self.dev(cnt, row_begin)
        out = self.dev(np.full(rows, SENTINEL, dtype=np.float32))
        gp = self.gp(k)
        self.torch.cuda.synchronize()
        st = self.L.as_knn_thresholds(self.sp, C.byref(gp), row_begin, row_begin + rows, float(nmax_all), kd[1], cd[1], out[1])
        assert st == expect, (st, self.lib.last_error())
        got, ok = self.back(out[0], 0, rows)
        assert ok, "as_knn_thresholds wrote outside its rows"
        return got

    def close(self):
        self.e.close()


@pytest.fixture(scope="module")
def spaces():
    made = {}

    def get(metric):
        if metric not in made:
            X, n = space_items()
            s = _Space(metric, X)
            np.testing.assert_array_equal(s.e.norms().cpu().numpy(), n)        # dyadic entries: the same bits in any order
            assert float(s.L.as_space_nmax(s.sp)) == n.max()
            made[metric] = s
        return made[metric]

    yield get
    for s in made.values():
        s.close()


def assert_slice(got, want, taking_part, label):
    """Rows taking part: count word, bound and the entries up to the new count, as bits.  The other rows: all six arrays
    as bits, the poisoned slots included."""
    np.testing.assert_array_equal(got[4], want[4], err_msg=label + ": count words")
    np.testing.assert_array_equal(_bits(got[5]), _bits(want[5]), err_msg=label + ": bounds")
    M = got[0].shape[1]
    look = (np.arange(M)[None, :] < (want[4] & 0xFFFF)[:, None]) | ~np.asarray(taking_part, dtype=bool)[:, None]
    for j, name in enumerate(("key", "dist", "gy", "idx")):
        np.testing.assert_array_equal(_bits(got[j])[look], _bits(want[j])[look], err_msg=label + ": " + name)


def assert_merge(got, want, label):
    np.testing.assert_array_equal(got["cnt"], want["cnt"], err_msg=label + ": counts")
    np.testing.assert_array_equal(got["idx"], want["idx"], err_msg=label + ": ids (-1 past the count)")
    k = got["idx"].shape[1]
    look = np.arange(k)[None, :] < want["cnt"][:, None]
    for name in ("key", "dist", "gy"):
        np.testing.assert_array_equal(_bits(got[name])[look], _bits(want[name])[look], err_msg=label + ": " + name)
    np.testing.assert_array_equal(got["flag"], want["flag"], err_msg=label + ": flags")
    band = np.where(want["flag"] != 0, want["band"], SENTINEL)          # written for exactly the flagged rows
    np.testing.assert_array_equal(_bits(got["band"]), _bits(band), err_msg=label + ": band")
    assert got["nflagged"] == want["nflagged"] == int(want["flag"].sum()), label


# ------------------------------------------------------------------------------------------------ A. fold
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("M,k", WIDTHS)
def test_fold_matches_the_model(spaces, M, k, metric):
    """Every pattern of fold_patterns, at 1 to 1027 rows, from row 0 and from row 3 (pointers offset to that row), in the
    three modes."""
    s = spaces(metric)
    assert int(s.L.as_knn_list_width(k)) == M
    for rows, row_begin, mode in FOLD_CONFIGS:
        c = fold_case(M, metric, rows, row_begin, mode)
        want = fold_expected(c, M, metric, mode)
        got = s.fold(k, row_begin, mode, c["nmax_b"], c["flag"], c["run"], c["blk"])
        part = np.ones(rows, dtype=bool) if mode == 0 else c["flag"] != 0
        assert_slice(got, want, part, "fold M=%d %s rows=%d from %d mode %d" % (M, metric, rows, row_begin, mode))


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("M,k", WIDTHS)
def test_chain_of_folds_matches_the_model_applied_as_often(spaces, M, k, metric):
    """Five blocks into an empty running list, then the second round's folds (mode 2 on the flagged rows, then mode 1):
    after every fold the running slice is the model's."""
    s = spaces(metric)
    blocks, nmax, modes, flag, n_rows = chain_case(M, metric)
    want = chain_expected(M, metric)
    run = empty_slice(len(flag), M)
    for step, (sl, nm, mode) in enumerate(zip(blocks, nmax, modes)):
        run = s.fold(k, 3, mode, nm, flag, run, sl)
        assert_slice(run, want[step], np.ones(len(flag), dtype=bool), "chain M=%d %s step %d" % (M, metric, step))
        # slots past the count are unspecified and never read: the next fold is fed the model's there
        look = np.arange(M)[None, :] < (want[step][4] & 0xFFFF)[:, None]
        run = tuple(np.where(look, g, w) for g, w in zip(run[:4], want[step][:4])) + (run[4], run[5])


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_fold_bound_under_the_default_coefficient(spaces, metric):
    """Without as_ring_i8_set the coefficient is (6 * 32 + 32) * 2^-24 + 3.03 * 2^-16, whose product with the norms is not
    exact.  The new bound is then the largest fp32 not above the rational b_t32 - e, or either fp32 neighbour of it: the
    fp64 rounding of the difference before the rounding down to fp32, or a fused multiply, can move the result by one fp32
    step and no more (the fp64 difference is off by at most half an fp64 ulp, far less than an fp32 step, so it lands in
    the same or an adjacent fp32 cell)."""
    s = spaces(metric)
    c = default_coef_case(metric)
    coef = oracle_np.ring_coef_default(DP)
    s.set_ring(False)
    try:
        got = s.fold(5, c["row_begin"], 0, c["nmax_b"], c["flag"], c["run"], c["blk"])
    finally:
        s.set_ring(True)
    np.testing.assert_array_equal(got[4], np.full(len(c["flag"]), 1 << 30, dtype=np.int32))
    steps = []
    for r in range(len(c["flag"])):
        e = Fraction(coef) * (Fraction(float(c["n_rows"][r])) + Fraction(c["nmax_b"])) if metric == "l2" else Fraction(coef)
        lo = f32_floor(Fraction(float(c["blk"][5][r])) - e)
        ok = [np.nextafter(lo, -F32_INF), lo, np.nextafter(lo, F32_INF)]
        steps.append([_bits(v).item() for v in ok].index(_bits(got[5][r]).item()) - 1 if got[5][r] in ok else 99)
    print("default coefficient, %s: fp32 steps off the exact floor: %s" % (metric, sorted(set(steps))))
    assert set(steps) <= {-1, 0, 1}, steps


# ------------------------------------------------------------------------------------------------ B. merge
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("M,k,nblocks,row_begin", MERGE_CONFIGS)
def test_merge_matches_the_model(spaces, M, k, nblocks, row_begin, metric):
    s = spaces(metric)
    c = merge_case(M, k, metric, nblocks, row_begin)
    want = merge_expected(c, M, k, metric)
    got = s.merge(k, c["eps"], row_begin, nblocks, c["slices"], c["block_nmax"])
    assert_merge(got, want, "merge M=%d %s nblocks=%d from %d" % (M, metric, nblocks, row_begin))
    # what the kinds promise, whatever the model says
    np.testing.assert_array_equal(got["flag"], [EXPECT_FLAG[kind] for kind in c["kinds"]])


def test_merge_refuses_more_blocks_than_its_lds_holds(spaces):
    """19 blocks of width 128 need 152 KiB for four rows: AS_EUNSUPPORTED, nothing launched (the outputs keep their fill)."""
    s = spaces("l2")
    slices = [empty_slice(4, 128) for _ in range(19)]
    got = s.merge(120, 1.0, 0, 19, slices, [1.0] * 19, expect=AS_EUNSUPPORTED)
    assert "LDS" in s.lib.last_error()
    assert (got["idx"] == -5).all() and (got["cnt"] == -5).all() and (got["flag"] == -5).all() and (got["band"] == SENTINEL).all()
    assert got["nflagged"] == 0


# ------------------------------------------------------------------------------------------------ C. thresholds
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("M,k", WIDTHS)
def test_thresholds_match_the_model(spaces, M, k, metric):
    s = spaces(metric)
    own = float(space_items()[1].max())
    for rows in THRESHOLD_ROWS:
        for row_begin in (0, 3):
            key, cnt, n_rows = thresholds_case(M, rows, row_begin)
            for nmax_all in (0.25, own + 7.5):          # below the space's own nmax (which then counts) and above it
                want = oracle_np.ring_thresholds(key, cnt, M, _metric(metric), COEF, n_rows, max(nmax_all, own))
                got = s.thresholds(k, row_begin, nmax_all, key, cnt)
                np.testing.assert_array_equal(_bits(got), _bits(want), err_msg="thresholds M=%d %s rows=%d from %d nmax_all=%g"
                                              % (M, metric, rows, row_begin, nmax_all))
                assert np.isinf(got[(cnt & 0xFFFF) < M]).all() and np.isfinite(got[(cnt & 0xFFFF) >= M]).all()


# ------------------------------------------------------------------------------------------------ D. refusals
def test_fold_and_merge_refuse_rows_outside_the_space(spaces):
    """Both kernels read the norm of row row_begin + r: a range that leaves the space is AS_EINVAL and launches nothing.
    The buffers are sized for the rows asked, and keep their contents."""
    s = spaces("l2")
    M, k = 32, 5
    for row_begin, rows in ((SPACE_N - 3, 4), (0, SPACE_N + 1)):          # row_end = n + 1
        run, blk = empty_slice(rows, M), empty_slice(rows, M)
        blk[4][:] = 1 << 30
        got = s.fold(k, row_begin, 0, 1.0, np.zeros(rows, dtype=np.int32), run, blk, expect=AS_EINVAL)
        assert "bad row range" in s.lib.last_error()
        assert_slice(got, run, np.zeros(rows, dtype=bool), "refused fold")
        res = s.merge(k, 1.0, row_begin, 0, [run], None, expect=AS_EINVAL)
        assert "bad row range" in s.lib.last_error()
        assert (res["cnt"] == -5).all() and (res["flag"] == -5).all()
    # row_begin > row_end
    gp = s.gp(k)
    run = [s.dev(a) for a in empty_slice(4, M)]
    outs = [s.dev(np.zeros(shape, dtype=dt)) for shape, dt in (((4, k), np.int32), ((4, k), np.float64), ((4, k), np.float64),
                                                                  ((4, k), np.float64), ((4,), np.int32), ((4,), np.int32), ((4,), np.float64))]
    nf = C.c_int64(0)
    s.torch.cuda.synchronize()
    assert s.L.as_knn_fold(s.sp, C.byref(gp), 8, 4, 0, 1.0, C.c_void_p(), *[p for _, p in run], *[p for _, p in run]) == AS_EINVAL
    assert s.L.as_knn_merge(s.sp, C.byref(gp), 8, 4, 0, *[p for _, p in run], C.c_void_p(), *[p for _, p in outs], C.byref(nf)) == AS_EINVAL
    assert s.L.as_knn_fold(s.sp, C.byref(gp), -1, 3, 0, 1.0, C.c_void_p(), *[p for _, p in run], *[p for _, p in run]) == AS_EINVAL
    # and a proper call still works afterwards
    c = fold_case(M, "l2", 5, 0, 0)
    assert_slice(s.fold(k, 0, 0, c["nmax_b"], c["flag"], c["run"], c["blk"]), fold_expected(c, M, "l2", 0), np.ones(5, dtype=bool), "after refusals")


# ------------------------------------------------------------------------------------------------ E. soundness
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_unflagged_rows_are_the_brute_force_lists(metric):
    """Truthful slices of 600 items in 5 uneven blocks: five folds and the folded merge, and the merge of the five slices.
    Every row a route does not flag equals the brute-force k nearest inside eps (ids, keys, count); both routes are the
    model's bit for bit, the folded route flags every row the unfolded one flags (its one rounding down per block only
    lowers the bound), and 20 - 80 % of the rows are flagged, so neither side of the property is empty."""
    c = soundness_case(metric)
    want_run, want_folded, want_unfolded = soundness_expected(metric)
    s = _Space(metric, c["X"])
    try:
        np.testing.assert_array_equal(s.e.norms().cpu().numpy(), c["n64"])
        run = empty_slice(SOUND_N, SOUND_M)
        for sl, nm in zip(c["slices"], c["block_nmax"]):
            run = s.fold(SOUND_K, 0, 0, nm, np.zeros(SOUND_N, dtype=np.int32), run, sl)
        assert_slice(run, want_run, np.ones(SOUND_N, dtype=bool), "soundness fold " + metric)
        folded = s.merge(SOUND_K, c["eps"], 0, 0, [run], None)
        unfolded = s.merge(SOUND_K, c["eps"], 0, len(c["slices"]), c["slices"], c["block_nmax"])
    finally:
        s.close()
    assert_merge(folded, want_folded, "soundness folded " + metric)
    assert_merge(unfolded, want_unfolded, "soundness unfolded " + metric)
    b_idx, b_key, b_cnt = c["brute"]
    for name, got in (("folded", folded), ("unfolded", unfolded)):
        ok = got["flag"] == 0
        share = 1.0 - ok.mean()
        print("soundness %s %s: %d of %d rows flagged" % (metric, name, int((~ok).sum()), SOUND_N))
        assert 0.2 <= share <= 0.8
        np.testing.assert_array_equal(got["cnt"][ok], b_cnt[ok])
        np.testing.assert_array_equal(got["idx"][ok], b_idx[ok])
        look = np.arange(SOUND_K)[None, :] < b_cnt[:, None]
        np.testing.assert_array_equal(_bits(got["key"])[ok[:, None] & look], _bits(b_key)[ok[:, None] & look])
    assert (folded["flag"] >= unfolded["flag"]).all()
