"""Row-sharded multi-GPU build and search: one process per GPU, torch.distributed
(backend "nccl" = RCCL over xGMI) for the exchange steps, the C ABI for every kernel.

Build   (DESIGN.md section 6): a rank keeps only ITS rows.  The raw shards travel round a ring (send to
        rank+1, receive from rank-1, double-buffered against the compute).  Every unordered pair of shards is computed
        ONCE (as_knn_block_pair: the keys of own rows x visiting columns serve both sides, the visiting rows' slice is
        sent home as one flat fp64 buffer), so the shards travel world // 2 hops; per block M exact candidates per row
        are folded into a running list, and after the last block as_knn_merge proves the k-NN lists exact.  Rows it
        cannot prove go round once more in collect mode (band pass), rows whose band overflows a third time (exact
        evaluation of every pair) -- both rounds collective.  Graph stage: every directed edge goes to the owner of
        its target row by one variable-count all-to-all, each rank builds ITS rows of the CSR; degrees, squared norms
        and energies (8 B per item each) are all-gathered, nothing of size N k is replicated.  `gather_lists=True`
        keeps the form with all-gathered lists and a replicated graph stage, `replicate=True` the round-1 form
        (all-gather of the whole item matrix).  Feature mode: the D x D Gram partials are all-gathered and summed.
Search: every rank scans its own rows, the k nearest-neighbour records and the top-k hit
        records (fixed-size structs of include/arrowspace_hip.h) are all-gathered and merged
        identically on every rank; two collectives of a few KB per query.

The host logic is engine-agnostic: `HipEngine` (this file) drives libarrowspace_hip.so;
tests inject a CPU engine to exercise the sharding logic under the gloo backend.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

KNN_REC_F64 = 6   # as_knn_rec = {int64 idx; double key, dist, gy, deg, ny}
HIT_REC_F64 = 2   # as_hit_rec = {int64 idx; double score}


def shard_bounds(n: int, world: int) -> list[int]:
    """Contiguous row ranges: rank r owns [b[r], b[r+1])."""
    base, rem = divmod(n, world)
    b = [0]
    for r in range(world):
        b.append(b[-1] + base + (1 if r < rem else 0))
    return b


def check_world_limits(graph_params, world: int):
    """A query merges world * k neighbour records and world * (topk + 1) hit records in one workgroup: refuse a
    combination beyond the library's capacities (1 024 and 8 208: e.g. k = 120 on 9 ranks) before anything is built."""
    from . import _lib
    L = _lib.load()
    gp = graph_params or {}
    k, topk = int(gp.get("k", 0)), int(gp.get("topk", 0))
    rec, hit = int(L.as_record_capacity(0)), int(L.as_record_capacity(1))
    if gp.get("lambda_mode", "item") != "feature" and world * k > rec:
        raise ValueError(f"graph_params['k']={k} on {world} ranks: a query merges world * k = {world * k} neighbour records, the maximum is {rec}")
    if world * (topk + 1) > hit:
        raise ValueError(f"graph_params['topk']={topk} on {world} ranks: a query merges world * (topk + 1) = {world * (topk + 1)} hit records, "
                         f"the maximum is {hit}")


def next_mode(mode: int, inexact: bool, overflow: int):
    """Escalation of one sharded search (every rank sees the same merged flags, so every rank takes the
    same step).  mode bits as in as_query_set_exact: 1 = fp64 scans, 2 = wavefront-list selection,
    4 = repair the k-NN candidates from the kept dots.  Returns None when the answer stands (or nothing
    stronger exists: fp64 + list selection).  Every step is strictly stronger, so a search takes at most
    four passes: 0 -> 4 -> 2 -> 3, or 0 -> 1 -> 5 -> 3."""
    if inexact and not mode & 1:
        # fp64 from scratch (the fp32 dots cannot be reused); a buffer that overflowed will overflow again,
        # so take the list path along with it
        return 3 if overflow or mode & 2 else 1
    if overflow & 1 and not mode & 6:
        # more than CAND_CAP rows inside eps: threshold repair, no rescan (the scorer ran on a truncated
        # neighbourhood, so its own overflow bit means nothing yet)
        return mode | 4
    if overflow and not mode & 2:
        return (mode | 2) & ~4                    # scorer buffer, or the repair itself overflowed: list path
    return None


class HipEngine:
    """Thin driver of the staged C ABI on this rank's GPU (torch tensors carry the pointers)."""

    def __init__(self, graph_params):
        import torch

        from . import _lib, _parse_graph_params

        self.torch = torch
        self._lib = _lib
        self.L = _lib.load()
        self.gp, self.op = _parse_graph_params(graph_params)
        self.op.device = torch.cuda.current_device()
        self.sp = C.c_void_p()
        self.gr = C.c_void_p()
        self.q = C.c_void_p()
        self._keep = []

    def _check(self, st):
        if st:
            from . import _raise
            _raise(st)

    def _fills_done(self):
        """torch fills its tensors on ITS current stream (ShardedIndex.stream), the library reads and writes them on the
        space's own: wait for that ONE stream.  Not torch.cuda.synchronize(): a device-wide wait would also sit out the
        ring hop that is in flight on RCCL's stream, and the hop is there to be hidden behind the kernels launched next."""
        self.torch.cuda.current_stream().synchronize()

    # ---- build
    def create_space(self, X):
        torch = self.torch
        assert X.is_cuda and X.is_contiguous() and X.dtype in (torch.float32, torch.float64)
        dt = self._lib.DTYPE_F32 if X.dtype == torch.float32 else self._lib.DTYPE_F64
        torch.cuda.current_stream().synchronize()
        self._check(self.L.as_space_create_dev(C.c_void_p(X.data_ptr()), dt, X.shape[0], X.shape[1], X.shape[1],
                                               C.byref(self.op), C.byref(self.sp)))
        self.n, self.d = int(X.shape[0]), int(X.shape[1])

    def knn_rows(self, r0, r1):
        torch = self.torch
        k, rows = int(self.gp.k), r1 - r0
        dev = torch.device("cuda", self.op.device)
        idx = torch.full((max(rows, 1), k), -1, dtype=torch.int32, device=dev)
        key = torch.zeros((max(rows, 1), k), dtype=torch.float64, device=dev)
        dist = torch.zeros_like(key)
        gy = torch.zeros_like(key)
        cnt = torch.zeros((max(rows, 1),), dtype=torch.int32, device=dev)
        torch.cuda.current_stream().synchronize()
        if rows > 0:
            self._check(self.L.as_knn_rows(self.sp, C.byref(self.gp), r0, r1, C.c_void_p(idx.data_ptr()),
                                           C.c_void_p(key.data_ptr()), C.c_void_p(dist.data_ptr()),
                                           C.c_void_p(gy.data_ptr()), C.c_void_p(cnt.data_ptr())))
        return idx[:rows], dist[:rows], gy[:rows], cnt[:rows]

    def graph_from_knn(self, idx, dist, gy, cnt):
        self.torch.cuda.current_stream().synchronize()
        self._check(self.L.as_graph_from_knn(self.sp, C.byref(self.gp), C.c_void_p(idx.data_ptr()),
                                             C.c_void_p(dist.data_ptr()), C.c_void_p(gy.data_ptr()),
                                             C.c_void_p(cnt.data_ptr()), C.byref(self.gr)))

    # ---- build without replication: visiting column blocks (ring)
    def ring_begin(self, nblocks):
        """Two slices of list memory: [0] the running fold of the blocks seen so far, [1] the block at hand."""
        torch = self.torch
        self.M = int(self.L.as_knn_list_width(int(self.gp.k)))
        if self.M < 0:
            raise ValueError(f"graph_params['k']={int(self.gp.k)} exceeds the supported maximum of 120")
        dev = torch.device("cuda", self.op.device)
        rows, M = max(self.n, 1), self.M
        self.p_key = torch.zeros((2, rows, M), dtype=torch.float64, device=dev)
        self.p_dist = torch.zeros_like(self.p_key)
        self.p_gy = torch.zeros_like(self.p_key)
        self.p_idx = torch.full((2, rows, M), -1, dtype=torch.int32, device=dev)
        self.p_cnt = torch.zeros((2, rows), dtype=torch.int32, device=dev)
        self.p_t32 = torch.zeros((2, rows), dtype=torch.float32, device=dev)
        self.nblocks, self._round2_first = nblocks, False
        # torch fills these on ITS stream, the library reads and writes them on its own: the fills must have run
        torch.cuda.synchronize()

    def open_block(self, X):
        """A visiting shard as a temporary space (ingested into the HBM layout the kernels read)."""
        torch = self.torch
        dt = self._lib.DTYPE_F32 if X.dtype == torch.float32 else self._lib.DTYPE_F64
        h = C.c_void_p()
        self._check(self.L.as_space_create_dev(C.c_void_p(X.data_ptr()), dt, X.shape[0], X.shape[1], X.shape[1],
                                               C.byref(self.op), C.byref(h)))
        return h

    def close_block(self, h):
        self.L.as_free_space(h)

    def own_block(self):
        return self.sp

    def block_nmax(self, h):
        return float(self.L.as_space_nmax(h))

    def _slice(self, b):
        return [C.c_void_p(t[b].data_ptr()) for t in (self.p_key, self.p_dist, self.p_gy, self.p_idx, self.p_cnt, self.p_t32)]

    def _fold(self, mode, nmax_b, flags=None):
        flag = C.c_void_p((self.l_flag if flags is None else flags).data_ptr()) if mode else C.c_void_p()
        self._check(self.L.as_knn_fold(self.sp, C.byref(self.gp), 0, self.n, mode, float(nmax_b), flag, *self._slice(0), *self._slice(1)))

    def knn_block(self, h, b, row_goff, col_goff):
        if self.n > 0:
            self._check(self.L.as_knn_block(self.sp, h, C.byref(self.gp), 0, self.n, row_goff, col_goff, *self._slice(1)))
            self._fold(0, self.block_nmax(h))

    # ---- symmetric ring: an unordered pair of blocks is computed once (as_knn_block_pair)
    def knn_thresholds(self, nmax_all):
        """Per-row upper bounds of the M-th smallest fp32 key, from the list folded so far (fp32 device tensor)."""
        torch = self.torch
        out = torch.full((max(self.n, 1),), float("inf"), dtype=torch.float32, device=torch.device("cuda", self.op.device))
        if self.n > 0:
            self._fills_done()
            self._check(self.L.as_knn_thresholds(self.sp, C.byref(self.gp), 0, self.n, float(nmax_all), C.c_void_p(self.p_key[0].data_ptr()),
                                                 C.c_void_p(self.p_cnt[0].data_ptr()), C.c_void_p(out.data_ptr())))
        return out[: self.n]

    def _slice_sections(self, P, nrows):
        """The sections of a packed slice: key / dist / gy fp64 [nrows, M], ids int32 [nrows, M], count int32 [nrows],
        drop bound fp32 [nrows] -- contiguous views of ONE flat fp64 buffer (the int32 / fp32 sections as bit patterns,
        each padded to a whole number of 8-byte words), so that the library writes the message in place and the receiver
        folds it in place."""
        torch = self.torch
        M, n = self.M, max(nrows, 1)
        w = n * M
        h = (n + 1) // 2
        o = [0, w, 2 * w, 3 * w, 3 * w + (w + 1) // 2, 3 * w + (w + 1) // 2 + h, 3 * w + (w + 1) // 2 + 2 * h]
        assert P.shape == (o[6],)
        return [P[o[0]:o[1]].view(n, M), P[o[1]:o[2]].view(n, M), P[o[2]:o[3]].view(n, M),
                P[o[3]:o[4]].view(torch.int32)[:w].view(n, M), P[o[4]:o[5]].view(torch.int32)[:n], P[o[5]:o[6]].view(torch.float32)[:n]]

    def slice_shape(self, nrows):
        n = max(nrows, 1)
        w = n * self.M
        return (3 * w + (w + 1) // 2 + 2 * ((n + 1) // 2),)

    def knn_block_pair(self, h, row0, row1, ct0, ct1, row_goff, col_goff, col_thr, ncols, row_thr=None):
        """Own rows [row0, row1) x the visiting block's column tiles [ct0, ct1): the own rows' slice is folded here; returns
        the visiting items' slice, packed for the way home (one flat fp64 tensor: _slice_sections)."""
        torch = self.torch
        dev = torch.device("cuda", self.op.device)
        P = torch.zeros(self.slice_shape(ncols), dtype=torch.float64, device=dev)
        qk, qd, qg, qi, qc, qt = self._slice_sections(P, ncols)
        qi.fill_(-1)
        qt.fill_(float("inf"))
        thr = col_thr.contiguous() if col_thr is not None else None
        rthr = row_thr.contiguous() if row_thr is not None else None     # the own rows' thresholds: [self.n] fp32
        assert rthr is None or (rthr.dtype == torch.float32 and rthr.shape[0] == self.n)
        self._fills_done()
        if self.n > 0 and ncols > 0:
            sl = [C.c_void_p(t[1].data_ptr() + row0 * t[1].stride(0) * t.element_size()) for t in
                  (self.p_key, self.p_dist, self.p_gy, self.p_idx, self.p_cnt, self.p_t32)]
            self._check(self.L.as_knn_block_pair(self.sp, h, C.byref(self.gp), row0, row1, ct0, ct1, row_goff, col_goff,
                                                 C.c_void_p(thr.data_ptr()) if thr is not None else C.c_void_p(),
                                                 C.c_void_p(rthr.data_ptr()) if rthr is not None else C.c_void_p(), *sl,
                                                 *[C.c_void_p(t.data_ptr()) for t in (qk, qd, qg, qi, qc, qt)]))
            if row1 > row0:
                self._fold_rows(row0, row1, self.block_nmax(h), 1)
        return P

    def _fold_rows(self, row0, row1, nmax_b, src_slice, ext=None):
        """Fold rows [row0, row1) of a block slice (slice `src_slice` of the list memory, or the external tensors `ext`)
        into the running list (slice 0)."""
        def off(t, r):
            return C.c_void_p(t.data_ptr() + r * t.stride(0) * t.element_size())
        run = [off(t[0], row0) for t in (self.p_key, self.p_dist, self.p_gy, self.p_idx, self.p_cnt, self.p_t32)]
        blk = [off(t, row0) for t in ext] if ext is not None else \
              [off(t[src_slice], row0) for t in (self.p_key, self.p_dist, self.p_gy, self.p_idx, self.p_cnt, self.p_t32)]
        self._check(self.L.as_knn_fold(self.sp, C.byref(self.gp), row0, row1, 0, float(nmax_b), C.c_void_p(), *run, *blk))

    def fold_slice(self, P, nmax_src):
        """A slice of MY rows that another rank computed (its items as my columns): into the running list."""
        if self.n == 0:
            return
        ext = self._slice_sections(P, self.n)
        self._fills_done()
        self._fold_rows(0, self.n, nmax_src, None, ext)

    def knn_merge(self, nmax=None, final=False):
        """Final lists from the folded slice; returns the number of rows not provably exact.  final: after the third round
        (every formerly overflowed row now holds exact per-block lists -- nothing is restored)."""
        torch = self.torch
        k, rows = int(self.gp.k), self.n
        dev = torch.device("cuda", self.op.device)
        first = not hasattr(self, "l_idx")
        if not first:
            keep = (self.l_idx, self.l_key, self.l_dist, self.l_gy, self.l_cnt, self.l_flag)
        self.l_idx = torch.full((max(rows, 1), k), -1, dtype=torch.int32, device=dev)
        self.l_key = torch.zeros((max(rows, 1), k), dtype=torch.float64, device=dev)
        self.l_dist = torch.zeros_like(self.l_key)
        self.l_gy = torch.zeros_like(self.l_key)
        self.l_cnt = torch.zeros((max(rows, 1),), dtype=torch.int32, device=dev)
        flag2 = torch.zeros((max(rows, 1),), dtype=torch.int32, device=dev)
        band = torch.zeros((max(rows, 1),), dtype=torch.float64, device=dev)
        nf = C.c_int64(0)
        torch.cuda.synchronize()
        if rows > 0:
            self._check(self.L.as_knn_merge(self.sp, C.byref(self.gp), 0, rows, 0, *self._slice(0), C.c_void_p(),
                                            *[C.c_void_p(t.data_ptr()) for t in (self.l_idx, self.l_key, self.l_dist, self.l_gy, self.l_cnt, flag2, band)],
                                            C.byref(nf)))
        if first:
            self.l_flag, self.l_band = flag2, band
        else:
            # second round: rows whose band overflowed somewhere (bit 1) keep their first-round list, unproven
            ov = (keep[5] & 2) != 0
            if bool(ov.any()) and not final:
                for new, old in zip((self.l_idx, self.l_key, self.l_dist, self.l_gy, self.l_cnt), keep[:5]):
                    new[ov] = old[ov]
            self.l_flag = flag2 if final else keep[5]
        return int(nf.value)

    def knn_block_band(self, h, b, row_goff, col_goff):
        ov = C.c_int64(0)
        if self.n > 0:
            self._check(self.L.as_knn_block_band(self.sp, h, C.byref(self.gp), 0, self.n, row_goff, col_goff,
                                                 C.c_void_p(self.l_flag.data_ptr()), C.c_void_p(self.l_band.data_ptr()),
                                                 *self._slice(1), C.byref(ov)))
            self._fold(1 if self._round2_first else 2, self.block_nmax(h))
            self._round2_first = True
        return int(ov.value)

    # ---- third round (last resort): rows whose band overflowed somewhere, by exact evaluation of every pair
    def overflowed_rows(self):
        """Rows left unproven by the second round (their band did not fit the collection buffers in some block)."""
        if self.n == 0 or not hasattr(self, "l_flag"):
            return 0
        self.l_over = ((self.l_flag[: self.n] & 2) != 0).to(self.torch.int32).contiguous()
        self._round3_first = False
        return int(self.l_over.sum().item())

    def knn_block_exact(self, h, b, row_goff, col_goff):
        if self.n > 0:
            self._fills_done()
            self._check(self.L.as_knn_block_exact(self.sp, h, C.byref(self.gp), 0, self.n, row_goff, col_goff, C.c_void_p(self.l_over.data_ptr()),
                                                  *self._slice(1)))
            self._fold(1 if self._round3_first else 2, self.block_nmax(h), self.l_over)
            self._round3_first = True

    def lists(self):
        rows = self.n
        return self.l_idx[:rows], self.l_dist[:rows], self.l_gy[:rows], self.l_cnt[:rows]

    def norms(self):
        """fp64 squared norms of the own rows (device tensor, copied out of the space)."""
        torch = self.torch
        out = torch.empty((max(self.n, 1),), dtype=torch.float64, device=torch.device("cuda", self.op.device))
        if self.n > 0:
            self._check(self.L.as_space_norms(self.sp, C.c_void_p(out.data_ptr())))
        return out[: self.n]

    def ring_end(self):
        """Drop the ring's list memory (before the graph stage allocates its CSR)."""
        for name in ("p_key", "p_dist", "p_gy", "p_idx", "p_cnt", "p_t32", "l_key", "l_band"):
            if hasattr(self, name):
                delattr(self, name)
        self.torch.cuda.empty_cache()

    def graph_from_knn_global(self, n_global, row_offset, idx, dist, gy, cnt, n64):
        self.torch.cuda.synchronize()
        self._check(self.L.as_graph_from_knn_global(self.sp, C.byref(self.gp), n_global, row_offset, C.c_void_p(idx.data_ptr()),
                                                    C.c_void_p(dist.data_ptr()), C.c_void_p(gy.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                                    C.c_void_p(n64.data_ptr()), C.byref(self.gr)))

    # ---- graph stage without replication: this rank's rows of the symmetrised graph
    # ---- ring build on the int8 images: every rank's measurement, then the ring-wide decision (as_ring_i8_stats / _set)
    def ring_i8_stats(self):
        out = (C.c_double * 3)()
        self._check(self.L.as_ring_i8_stats(self.sp, C.cast(out, C.c_void_p)))
        return [float(out[0]), float(out[1]), float(out[2])]

    def ring_i8_set(self, u_max, v_max, usable):
        self._check(self.L.as_ring_i8_set(self.sp, float(u_max), float(v_max), 1 if usable else 0))
        return bool(self.L.as_ring_i8(self.sp))

    def edge_bucket(self, idx, dist, gy, cnt, row0, bounds):
        """The lists' directed edges bucketed by the owner of their target (as_edges_bucket: count / scan / scatter kernels)
        -> (ints [E, 2] int32, reals [E, 2] float64, per-rank counts)."""
        torch = self.torch
        rows, k = int(idx.shape[0]), int(idx.shape[1])
        world = len(bounds) - 1
        idx, dist, gy, cnt = idx.contiguous(), dist.contiguous(), gy.contiguous(), cnt.contiguous()
        assert idx.dtype == torch.int32 and cnt.dtype == torch.int32 and dist.dtype == torch.float64 and gy.dtype == torch.float64
        ints = torch.empty((max(rows * k, 1), 2), dtype=torch.int32, device=idx.device)
        reals = torch.empty((max(rows * k, 1), 2), dtype=torch.float64, device=idx.device)
        bh = (C.c_int64 * (world + 1))(*[int(b) for b in bounds])
        counts = (C.c_int64 * world)()
        self._check(self.L.as_edges_bucket(C.c_void_p(idx.data_ptr()), C.c_void_p(dist.data_ptr()), C.c_void_p(gy.data_ptr()),
                                           C.c_void_p(cnt.data_ptr()), rows, k, int(row0), C.cast(bh, C.c_void_p), world,
                                           C.c_void_p(ints.data_ptr()), C.c_void_p(reals.data_ptr()), C.cast(counts, C.c_void_p),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        send = [int(v) for v in counts]
        total = sum(send)
        return ints[:total], reals[:total], send

    def graph_shard_csr(self, n_global, row_offset, idx, dist, gy, cnt, in_row, in_col, in_dist, in_gy):
        """-> the degrees of this rank's rows (device tensor, a copy)."""
        torch = self.torch
        torch.cuda.synchronize()
        keep = [t.contiguous() for t in (idx, dist, gy, cnt, in_row, in_col, in_dist, in_gy)]
        assert keep[0].dtype == torch.int32 and keep[4].dtype == torch.int32 and keep[5].dtype == torch.int32
        self._check(self.L.as_graph_shard_csr(self.sp, C.byref(self.gp), n_global, row_offset, *[C.c_void_p(t.data_ptr()) for t in keep[:4]],
                                              int(keep[4].shape[0]), *[C.c_void_p(t.data_ptr()) for t in keep[4:]], C.byref(self.gr)))
        return self._graph_vec(self.L.as_graph_deg_copy)

    def _graph_vec(self, fn):
        torch = self.torch
        out = torch.empty((max(self.n, 1),), dtype=torch.float64, device=torch.device("cuda", self.op.device))
        if self.n > 0:
            self._check(fn(self.gr, C.c_void_p(out.data_ptr())))
        return out[: self.n]

    def graph_shard_energy(self, deg_global, n64_global):
        """-> the energies E of this rank's rows (device tensor, a copy)."""
        self.torch.cuda.synchronize()
        self._check(self.L.as_graph_shard_energy(self.sp, self.gr, C.c_void_p(deg_global.data_ptr()), C.c_void_p(n64_global.data_ptr())))
        return self._graph_vec(self.L.as_graph_energy_copy)

    def graph_shard_lambdas(self, E_global):
        self.torch.cuda.synchronize()
        self._check(self.L.as_graph_shard_lambdas(self.sp, self.gr, C.c_void_p(E_global.data_ptr()), int(E_global.shape[0])))

    # ---- search
    def query_open(self):
        torch = self.torch
        self._check(self.L.as_query_create(self.sp, self.gr, C.byref(self.q)))
        self.k = int(self.L.as_query_knn_capacity(self.q))
        self.hcap = int(self.L.as_query_hit_capacity(self.q))
        dev = torch.device("cuda", self.op.device)
        self.knn_local = torch.zeros((self.k, KNN_REC_F64), dtype=torch.float64, device=dev)
        self.hits_local = torch.zeros((self.hcap, HIT_REC_F64), dtype=torch.float64, device=dev)
        self._check(self.L.as_query_bind_records(self.q, C.c_void_p(self.knn_local.data_ptr()),
                                                 C.c_void_p(self.hits_local.data_ptr())))
        # run the query kernels on torch's current stream: RCCL collectives order against it
        self.L.as_query_set_stream(self.q, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        self.topk = self.hcap - 1
        self._idx = np.empty(max(self.topk, 1), dtype=np.int64)
        self._sc = np.empty(max(self.topk, 1), dtype=np.float64)

    def set_mode(self, mode):
        self.L.as_query_set_exact(self.q, int(mode))

    # ---- the two per-query exchange steps issued by the library (RCCL from C++, as_comm.hip): one host call per query
    def comm_available(self):
        return bool(self.L.as_comm_available())

    def comm_unique_id(self):
        buf = (C.c_char * 128)()
        self._check(self.L.as_comm_unique_id(C.cast(buf, C.c_void_p)))
        return bytes(buf)

    def comm_create(self, uid: bytes, rank: int, world: int):
        """Collective over the ranks of the index.  The query keeps its own record buffers and its own stream."""
        self.comm = C.c_void_p()
        buf = (C.c_char * 128).from_buffer_copy(uid)
        self._check(self.L.as_comm_create(C.cast(buf, C.c_void_p), rank, world, int(self.op.device), C.byref(self.comm)))
        self.qs = C.c_void_p()
        self._check(self.L.as_query_create(self.sp, self.gr, C.byref(self.qs)))
        self._check(self.L.as_query_set_comm(self.qs, self.comm))
        self.L.as_query_set_x1(self.qs, self.L.as_query_x1_enabled(self.q))   # (what the ranks agreed on for self.q)
        self._sidx = np.empty(max(self.topk, 1), dtype=np.int64)
        self._ssc = np.empty(max(self.topk, 1), dtype=np.float64)

    def search_staged(self, q, tau, r0, r1):
        """-> (hits, lambda_q, zero_lambda): scan, both exchanges, merge and escalation behind one call."""
        qq = np.ascontiguousarray(q, dtype=np.float64)
        ln, lq = C.c_int64(0), C.c_double(0.0)
        st = self.L.as_query_search_staged(self.qs, qq.ctypes.data_as(C.c_void_p), qq.shape[0], r0, r1, float(tau),
                                           self._sidx.ctypes.data_as(C.c_void_p), self._ssc.ctypes.data_as(C.c_void_p), C.byref(ln), C.byref(lq))
        if st not in (self._lib.AS_OK, self._lib.AS_EZEROLAMBDA):
            self._check(st)
        n = ln.value
        return list(zip(self._sidx[:n].tolist(), self._ssc[:n].tolist())), float(lq.value), st == self._lib.AS_EZEROLAMBDA

    def query_scan(self, q, r0, r1):
        self._q = np.ascontiguousarray(q, dtype=np.float64)
        self._check(self.L.as_query_scan(self.q, self._q.ctypes.data_as(C.c_void_p), self._q.shape[0], r0, r1))

    # ---- one exchange per query (as_query_x1_*): this rank's block -> all-gather -> the same finish on every rank
    def x1_usable(self, tau):
        return bool(self.L.as_query_x1_usable(self.q, float(tau)))

    def x1_enabled(self):
        """This rank's own switch of the one-exchange pass (ARROWSPACE_STAGED_X1 when the workspace was made)."""
        return bool(self.L.as_query_x1_enabled(self.q))

    def x1_set_enabled(self, enabled):
        """The switch the ranks agreed on, for every query workspace of this engine."""
        self.L.as_query_set_x1(self.q, 1 if enabled else 0)
        if getattr(self, "qs", None):
            self.L.as_query_set_x1(self.qs, 1 if enabled else 0)

    def x1_begin(self, q, tau, r0, r1, world):
        torch = self.torch
        if getattr(self, "_x1_world", None) != world:
            nbytes = int(self.L.as_query_x1_bytes(self.q, int(world)))
            self.x1_send = torch.zeros((nbytes // 8,), dtype=torch.float64, device=torch.device("cuda", self.op.device))
            self._x1_world = world
        self._q = np.ascontiguousarray(q, dtype=np.float64)
        self._check(self.L.as_query_x1_begin(self.q, self._q.ctypes.data_as(C.c_void_p), self._q.shape[0], r0, r1, float(tau),
                                             C.c_void_p(self.x1_send.data_ptr()), int(world)))
        return self.x1_send

    def x1_finish(self, blocks_all, tau, world):
        """-> (hits, lambda_q, zero_lambda, inexact, overflow, redo); redo: run the query through the two-exchange steps."""
        ln, lq = C.c_int64(0), C.c_double(0.0)
        st = self.L.as_query_x1_finish(self.q, C.c_void_p(blocks_all.data_ptr()), int(world), float(tau),
                                       self._idx.ctypes.data_as(C.c_void_p), self._sc.ctypes.data_as(C.c_void_p), C.byref(ln), C.byref(lq))
        if st not in (self._lib.AS_OK, self._lib.AS_EZEROLAMBDA):
            self._check(st)
        ki, si = C.c_int32(0), C.c_int32(0)
        self.L.as_query_flags(self.q, C.byref(ki), C.byref(si))
        hits = [(int(self._idx[t]), float(self._sc[t])) for t in range(ln.value)]
        return (hits, float(lq.value), st == self._lib.AS_EZEROLAMBDA, bool(ki.value & 1), 1 if ki.value & 2 else 0,
                bool(self.L.as_query_x1_redo(self.q)))

    def x1_set_coarse(self, allowed):
        self.L.as_query_set_coarse(self.q, 1 if allowed else 0)

    def x1_passes(self, library=False):
        return int(self.L.as_query_x1_passes(self.qs if library else self.q))

    def query_lambda(self, knn_all):
        self._check(self.L.as_query_lambda(self.q, C.c_void_p(knn_all.data_ptr()), knn_all.shape[0]))

    def query_score(self, tau):
        self._check(self.L.as_query_score(self.q, float(tau)))

    def query_finish(self, hits_all):
        ln, lq = C.c_int64(0), C.c_double(0.0)
        st = self.L.as_query_finish(self.q, C.c_void_p(hits_all.data_ptr()), hits_all.shape[0],
                                    self._idx.ctypes.data_as(C.c_void_p), self._sc.ctypes.data_as(C.c_void_p),
                                    C.byref(ln), C.byref(lq))
        ki, si = C.c_int32(0), C.c_int32(0)
        self.L.as_query_flags(self.q, C.byref(ki), C.byref(si))
        inexact = bool((ki.value & 1) or (si.value & 1))
        overflow = (1 if ki.value & 2 else 0) | (2 if si.value & 2 else 0)   # bit0: k-NN buffer, bit1: scorer buffer
        if st not in (self._lib.AS_OK, self._lib.AS_EZEROLAMBDA):
            self._check(st)
        hits = [(int(self._idx[t]), float(self._sc[t])) for t in range(ln.value)]
        return hits, float(lq.value), st == self._lib.AS_EZEROLAMBDA, inexact, overflow

    # ---- feature mode (lambda on the F x F feature-space Laplacian): Gram partials add up over the shards
    def feature_mode(self):
        return int(self.op.lambda_mode) == self._lib.LAMBDA_MODES["feature"]

    def feat_gram(self):
        torch = self.torch
        g = torch.zeros((self.d, self.d), dtype=torch.float64, device=torch.device("cuda", self.op.device))
        torch.cuda.synchronize()   # (the zero fill runs on torch's stream, the library writes on its own: a late fill would wipe the result)
        if self.n > 0:
            self._check(self.L.as_feat_gram(self.sp, 0, self.n, C.c_void_p(g.data_ptr())))
        return g

    def feat_graph(self, gram):
        self.torch.cuda.synchronize()
        self._check(self.L.as_feat_graph(self.sp, C.byref(self.gp), C.c_void_p(gram.data_ptr()), C.byref(self.gr)))

    def feat_energy(self):
        torch = self.torch
        dev = torch.device("cuda", self.op.device)
        E = torch.zeros((max(self.n, 1),), dtype=torch.float64, device=dev)
        G = torch.zeros_like(E)
        torch.cuda.synchronize()   # as in feat_gram
        if self.n > 0:
            self._check(self.L.as_feat_energy(self.sp, self.gr, 0, self.n, C.c_void_p(E.data_ptr()), C.c_void_p(G.data_ptr())))
        return E[: self.n], G[: self.n]

    def feat_lambdas_global(self, E, G, n_global, row_offset):
        self.torch.cuda.synchronize()
        self._check(self.L.as_feat_lambdas_global(self.sp, self.gr, C.c_void_p(E.data_ptr()), C.c_void_p(G.data_ptr()), n_global, row_offset))

    # ---- persistence: this rank's shard + the graph, one file per rank
    def save(self, path):
        self._check(self.L.as_index_save(self.sp, self.gr, os.fsencode(path)))

    def load(self, path):
        self._check(self.L.as_index_load(os.fsencode(path), C.byref(self.op), C.byref(self.sp), C.byref(self.gr)))
        self.n, self.d = int(self.L.as_nitems(self.sp)), int(self.L.as_nfeatures(self.sp))
        return int(self.L.as_space_row_offset(self.sp)), int(self.L.as_graph_nitems(self.gr))

    # ---- batched staged search (32 slots per pass)
    def batch_open(self):
        torch = self.torch
        self.qb = C.c_void_p()
        self._check(self.L.as_query_create_batch(self.sp, self.gr, C.byref(self.qb)))
        self.cap = int(self.L.as_query_slots(self.qb))
        dev = torch.device("cuda", self.op.device)
        self.knn_local_b = torch.zeros((self.cap, self.k, KNN_REC_F64), dtype=torch.float64, device=dev)
        self.hits_local_b = torch.zeros((self.cap, self.hcap, HIT_REC_F64), dtype=torch.float64, device=dev)
        self._check(self.L.as_query_bind_records(self.qb, C.c_void_p(self.knn_local_b.data_ptr()),
                                                 C.c_void_p(self.hits_local_b.data_ptr())))
        self.L.as_query_set_stream(self.qb, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        self._bidx = np.empty((self.cap, max(self.topk, 1)), dtype=np.int64)
        self._bsc = np.empty((self.cap, max(self.topk, 1)), dtype=np.float64)
        return self.cap

    def query_scan_batch(self, Q, r0, r1):
        self._qb = np.ascontiguousarray(Q, dtype=np.float64)
        self._check(self.L.as_query_scan_batch(self.qb, self._qb.ctypes.data_as(C.c_void_p), self._qb.shape[0], self._qb.shape[1], r0, r1))

    def query_lambda_batch(self, knn_all, nranks):
        self._check(self.L.as_query_lambda_batch(self.qb, C.c_void_p(knn_all.data_ptr()), nranks))

    def query_score_batch(self, tau):
        self._check(self.L.as_query_score_batch(self.qb, float(tau)))

    def query_finish_batch(self, hits_all, nranks, nb):
        """-> per query (hits | None when it has to be rerun query by query, lambda_q, zero_lambda)."""
        ln = np.zeros(self.cap, dtype=np.int64)
        lq = np.zeros(self.cap, dtype=np.float64)
        st = np.zeros(self.cap, dtype=np.int32)
        self._check(self.L.as_query_finish_batch(self.qb, C.c_void_p(hits_all.data_ptr()), nranks, self._bidx.ctypes.data_as(C.c_void_p),
                                                 self._bsc.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p),
                                                 lq.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)))
        out = []
        il, sl, ll, ql, stl = self._bidx[:nb].tolist(), self._bsc[:nb].tolist(), ln.tolist(), lq.tolist(), st.tolist()
        for b in range(nb):
            if stl[b] == -1:
                out.append((None, 0.0, False))
            else:
                out.append((list(zip(il[b][: ll[b]], sl[b][: ll[b]])), ql[b], stl[b] == self._lib.AS_EZEROLAMBDA))
        return out

    def lambdas(self):
        out = np.empty(self.n, dtype=np.float64)
        self._check(self.L.as_lambdas(self.sp, out.ctypes.data_as(C.c_void_p)))
        return out

    def csr(self):
        """(indptr, indices, values) of this rank's rows of the Laplacian, diagonal included, column ids global."""
        rows, nnz = int(self.L.as_nnodes(self.gr)), int(self.L.as_graph_nnz(self.gr))
        ip = np.zeros(rows + 1, dtype=np.int64)
        ix = np.zeros(max(nnz, 1), dtype=np.int64)
        v = np.zeros(max(nnz, 1), dtype=np.float64)
        self._check(self.L.as_graph_csr(self.gr, ip.ctypes.data_as(C.c_void_p), ix.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)))
        return ip, ix[:nnz], v[:nnz]

    def degrees(self):
        return self._graph_vec(self.L.as_graph_deg_copy).cpu().numpy()

    def stats(self):
        out = np.zeros(10, dtype=np.float64)
        self.L.as_build_stats(self.gr, out.ctypes.data_as(C.c_void_p), 10)
        keys = ("ingest_s", "knn_mfma_s", "refine_s", "fallback_s", "graph_s", "total_s", "fallback_rows", "mfma_flops",
                "unproven_rows", "band_rows")
        return dict(zip(keys, out.tolist()))

    def tau0(self):
        return float(self.L.as_graph_tau0(self.gr))

    def scan_us(self, q=None):
        out = np.zeros(3, dtype=np.float64)
        self.L.as_query_stats(q if q is not None else self.q, out.ctypes.data_as(C.c_void_p), 3)
        return float(out[0])

    def close(self):
        if getattr(self, "qs", None):
            self.L.as_query_free(self.qs)
            self.qs = None
        if getattr(self, "comm", None):
            self.L.as_comm_free(self.comm)
            self.comm = None
        if getattr(self, "qb", None):
            self.L.as_query_free(self.qb)
            self.qb = C.c_void_p()
        if self.q:
            self.L.as_query_free(self.q)
            self.q = C.c_void_p()
        if self.gr:
            self.L.as_free_graph(self.gr)
            self.gr = C.c_void_p()
        if self.sp:
            self.L.as_free_space(self.sp)
            self.sp = C.c_void_p()


class ShardedIndex:
    """Host logic of the row-sharded index; identical results on every rank."""

    library_exchange = True      # single-query searches: the library issues the two exchange steps itself (RCCL from C++)

    def __init__(self):
        self.engine = None
        self._gbuf = {}
        self.stream = None
        self.force_collectives = False
        self._lib_comm = False

    def _setup_library_exchange(self):
        """A communicator of this index's ranks inside the library (as_comm.hip): search() is then ONE host call per query --
        no Python between the scan, the two all-gathers and the merge.  Needs real RCCL ranks (one GPU per rank);
        ARROWSPACE_PY_COLLECTIVES=1 keeps the torch.distributed path (A/B runs)."""
        e = self.engine
        self._agree_query_switches()
        # (what decides here is the same on every rank: the class, the engine type, the group's backend)
        if not (self.library_exchange and self._collective() and hasattr(e, "comm_create")):
            return
        if self.dist.get_backend(self.group) != "nccl":
            return
        torch = self.torch
        dev = torch.device("cuda", e.op.device)
        # as_comm_create is collective: every rank must be able to take part (a rank without librccl would leave the others
        # waiting in ncclCommInitRank) -- agree first.  Whatever may DIFFER between ranks -- librccl on the box, this rank's
        # environment (ARROWSPACE_PY_COLLECTIVES) -- goes into the vote, never into a return in front of it: ranks that take
        # different branches here issue different collectives for every query that follows.
        mine = e.comm_available() and not os.environ.get("ARROWSPACE_PY_COLLECTIVES")
        ok = torch.tensor([1 if mine else 0], dtype=torch.int32, device=dev)
        self.dist.all_reduce(ok, op=self.dist.ReduceOp.MIN, group=self.group)
        if int(ok.item()) == 0:
            return
        uid = torch.zeros(128, dtype=torch.uint8, device=dev)
        if self.rank == 0:
            uid.copy_(torch.frombuffer(bytearray(e.comm_unique_id()), dtype=torch.uint8))
        self.dist.broadcast(uid, self.dist.get_global_rank(self.group, 0) if self.group is not None else 0, group=self.group)
        try:
            e.comm_create(bytes(uid.cpu().numpy().tobytes()), self.rank, self.world)
            made = 1
        except (RuntimeError, ValueError) as err:   # a rank that cannot join: every rank must learn it
            made = 0
            if self.rank == 0:
                import sys
                print("[pyarrowspace] library-side exchange not available (%s): torch.distributed collectives stay" % err, file=sys.stderr)
        ok.fill_(made)
        self.dist.all_reduce(ok, op=self.dist.ReduceOp.MIN, group=self.group)
        self._lib_comm = int(ok.item()) == 1     # all ranks or none: the two paths issue different collectives

    def _agree_query_switches(self):
        """What a rank's ENVIRONMENT may switch about the query path -- the one-exchange pass, ARROWSPACE_STAGED_X1 -- decides
        which collectives a search issues (one all-gather of blocks, or two of records): agreed once over the ranks when
        the query is opened (MIN: any rank that has it off switches it off for all), never read per call and per rank."""
        e = self.engine
        if not (hasattr(e, "x1_enabled") and hasattr(e, "x1_set_enabled")):
            return
        mine = 1.0 if e.x1_enabled() else 0.0
        if self._collective():
            torch = self.torch
            t = torch.tensor([mine], dtype=torch.float64, device=e.knn_local.device)
            mine = float(self._gather_fixed(t).min().item())
        e.x1_set_enabled(mine > 0.0)

    # ---- collectives
    def _collective(self):
        return self.world > 1 or self.force_collectives

    def _gather_rows(self, t, counts):
        """t: this rank's [rows_r, ...] tensor -> concatenation over ranks, [sum(counts), ...]."""
        torch = self.torch
        world = len(counts)
        if not self._collective():
            return t
        mx = max(max(counts), 1)
        if t.is_cuda and all(c == mx for c in counts):
            # RCCL all-gather straight into the final buffer (equal shards: no padding, no copies)
            out = torch.empty((world * mx,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            self.dist.all_gather_into_tensor(out, t.contiguous(), group=self.group)
            return out
        pad = torch.zeros((mx,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        pad[: t.shape[0]] = t
        if t.is_cuda:
            buf = torch.empty((world * mx,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            self.dist.all_gather_into_tensor(buf, pad, group=self.group)
            parts = [buf[r * mx : r * mx + counts[r]] for r in range(world)]
        else:
            full = [torch.empty_like(pad) for _ in range(world)]
            self.dist.all_gather(full, pad, group=self.group)
            parts = [full[r][: counts[r]] for r in range(world)]
        return torch.cat(parts, dim=0)

    def _exchange_start(self, send, recv, nxt_rank, prv_rank):
        """One ring hop: `send` goes to the next rank, `recv` is filled by the previous one (RCCL send/recv)."""
        dist = self.dist
        return dist.batch_isend_irecv([dist.P2POp(dist.isend, send, nxt_rank, group=self.group),
                                       dist.P2POp(dist.irecv, recv, prv_rank, group=self.group)])

    def _exchange_wait(self, reqs):
        for r in reqs:
            r.wait()

    def _all_to_all(self, t, recv_counts, send_counts):
        """Variable-count all-to-all over dim 0 (RCCL grouped send/recv): rows [sum(send_counts[:r]), ...) of t go to rank r;
        counts None: one row each way."""
        rows = t.shape[0] if recv_counts is None else sum(recv_counts)
        out = self.torch.empty((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        self.dist.all_to_all_single(out, t.contiguous(), output_split_sizes=recv_counts, input_split_sizes=send_counts, group=self.group)
        return out

    def _gather_fixed(self, t, persistent=False):
        """All-gather of equally shaped tensors.  persistent: t is one of the engine's record tensors, alive as long as
        the index -- its [world * rows, ...] output buffer is allocated once and reused by every query; build-time
        temporaries (Gram partials, thresholds) take a fresh buffer that dies with them."""
        torch = self.torch
        if not self._collective():
            return t
        if t.is_cuda:
            key = (t.data_ptr(), tuple(t.shape), t.dtype)
            out = self._gbuf.get(key) if persistent else None
            if out is None:
                out = torch.empty((self.world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
                if persistent:
                    self._gbuf[key] = out
            self.dist.all_gather_into_tensor(out, t, group=self.group)
            return out
        parts = [torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(parts, t, group=self.group)
        return torch.cat(parts, dim=0)

    @classmethod
    def build(cls, graph_params, X_shard, dist=None, group=None, engine=None, force_collectives=False, replicate=False,
              gather_lists=False):
        """X_shard: this rank's contiguous block of rows (torch tensor on this rank's device,
        fp32 or fp64).  Ranks hold consecutive blocks in rank order.  replicate=True: all-gather the
        whole item matrix onto every rank first (round-1 form; twice the HBM).  gather_lists=True: ring k-NN, but the
        lists of all items on every rank and the graph stage replicated (O(N k) per rank)."""
        import contextlib

        import torch

        import time

        self = cls()
        self.torch, self.dist, self.group = torch, dist, group
        self.world = dist.get_world_size(group) if dist is not None else 1
        self.rank = dist.get_rank(group) if dist is not None else 0
        self.phase_s = {}          # seconds per phase of this rank's build (host clock; every phase ends on a host wait)
        _t = [time.perf_counter()]

        def lap(name):
            now = time.perf_counter()
            self.phase_s[name] = self.phase_s.get(name, 0.0) + now - _t[0]
            _t[0] = now

        self._lap = lap
        check_world_limits(graph_params, self.world)      # before any upload or GPU work
        self.force_collectives = bool(force_collectives) and dist is not None
        self.engine = engine if engine is not None else HipEngine(graph_params)
        self.replicated = bool(replicate) or not hasattr(self.engine, "knn_block")
        # CUDA: kernels and RCCL collectives are ordered on ONE dedicated, non-default stream
        # (the legacy default stream has handle 0 and cannot be handed to the library)
        self.stream = torch.cuda.Stream() if X_shard.is_cuda else None
        ctx = torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream())
        with ctx:
            rows = int(X_shard.shape[0])
            if self.world > 1:
                c = torch.tensor([rows], dtype=torch.int64, device=X_shard.device)
                cs = [torch.zeros_like(c) for _ in range(self.world)]
                dist.all_gather(cs, c, group=group)
                counts = [int(v.item()) for v in cs]
            else:
                counts = [rows]
            self.counts = counts
            self.bounds = [0]
            for v in counts:
                self.bounds.append(self.bounds[-1] + v)
            self.n = self.bounds[-1]
            self.r0, self.r1 = self.bounds[self.rank], self.bounds[self.rank + 1]
            if min(counts) == 0 and isinstance(self.engine, HipEngine):
                self.replicated = True      # a rank without rows has no space of its own to scan: keep the all-gather form
            if getattr(self.engine, "feature_mode", lambda: False)():
                # lambda on the F x F feature-space Laplacian: the D x D Gram partials of the shards add up (all-gather +
                # fixed-order sum: the same bits on every rank), the feature graph is built redundantly (D nodes), the
                # energies are local, tau0 needs all of them (all-gather of 16 B per item).  No item ever leaves its rank.
                if min(counts) == 0:
                    raise ValueError("feature mode needs at least one item on every rank")
                self.replicated = False
                X_shard = X_shard.contiguous()
                self._sync()
                self.engine.create_space(X_shard)
                g = self.engine.feat_gram()
                if self._collective():
                    parts = self._gather_fixed(g).reshape(self.world, g.shape[0], g.shape[1])
                    g = parts[0].clone()
                    for r in range(1, self.world):
                        g += parts[r]
                self._sync()
                self.engine.feat_graph(g)
                E, G = self.engine.feat_energy()
                E = self._gather_rows(E.contiguous(), counts).contiguous()
                G = self._gather_rows(G.contiguous(), counts).contiguous()
                self._sync()
                self.engine.feat_lambdas_global(E, G, self.n, self.r0)
                self.scan_rows = (0, rows)
                self.engine.query_open()
                self._setup_library_exchange()
                return self
            if self.replicated:
                X_full = self._gather_rows(X_shard.contiguous(), counts).contiguous()
                self._sync()
                self.engine.create_space(X_full)
                del X_full
                idx, dst, gy, cnt = self.engine.knn_rows(self.r0, self.r1)
                self.scan_rows = (self.r0, self.r1)      # the space holds every item: this rank scans its slice
            else:
                X_shard = X_shard.contiguous()
                self._sync()
                self.engine.create_space(X_shard)
                lap("ingest")
                idx, dst, gy, cnt = self._ring_knn(X_shard)
                self.scan_rows = (0, rows)               # the space holds this rank's rows only; ids come out global
            if self.replicated:
                idx = self._gather_rows(idx, counts).contiguous()
                dst = self._gather_rows(dst, counts).contiguous()
                gy = self._gather_rows(gy, counts).contiguous()
                cnt = self._gather_rows(cnt, counts).contiguous()
                self._sync()
                self.engine.graph_from_knn(idx, dst, gy, cnt)
            elif gather_lists or not hasattr(self.engine, "graph_shard_csr"):
                # round-2a form: the lists of all items on every rank, the graph stage replicated
                idx = self._gather_rows(idx, counts).contiguous()
                dst = self._gather_rows(dst, counts).contiguous()
                gy = self._gather_rows(gy, counts).contiguous()
                cnt = self._gather_rows(cnt, counts).contiguous()
                n64 = self._gather_rows(self.engine.norms(), counts).contiguous()
                self._sync()
                self.engine.graph_from_knn_global(self.n, self.r0, idx, dst, gy, cnt, n64)
            else:
                # one exchange step.  Every directed edge goes to the owner of its target row (variable-count
                # all-to-all, 24 B per edge), each rank symmetrises and weighs ITS rows; what the energies need of the
                # neighbours -- degree and squared norm -- and what tau0 needs -- every energy -- are O(N) vectors,
                # all-gathered (8 B per item each).  Nothing of size N k is replicated.
                inc = self._exchange_edges(idx, dst, gy, cnt)
                self._sync()
                lap("edge_exchange")
                deg = self.engine.graph_shard_csr(self.n, self.r0, idx, dst, gy, cnt, *inc)
                del inc
                lap("graph_csr")
                deg_g = self._gather_rows(deg.contiguous(), counts).contiguous()
                n64 = self._gather_rows(self.engine.norms().contiguous(), counts).contiguous()
                self._sync()
                E = self.engine.graph_shard_energy(deg_g, n64)
                del deg_g, n64
                E_g = self._gather_rows(E.contiguous(), counts).contiguous()
                self._sync()
                self.engine.graph_shard_lambdas(E_g)
                lap("energies_lambdas")
            self.engine.query_open()
            self._setup_library_exchange()
            lap("query_open")
        return self

    def _exchange_edges(self, idx, dst, gy, cnt):
        """The directed edges i -> j of this rank's lists, delivered to the owner of row j: returns what arrived here
        (from every rank, this one included) as (row local to this rank int32, source item id int32, dist, gy)."""
        torch, dist = self.torch, self.dist
        rows, k = int(idx.shape[0]), int(idx.shape[1])
        dev = idx.device
        if idx.is_cuda and hasattr(self.engine, "edge_bucket") and idx.dtype == torch.int32 and cnt.dtype == torch.int32 and self.world <= 64 \
                and not os.environ.get("ARROWSPACE_TORCH_EDGES"):
            # count / scan / scatter kernels of the library (as_edges.hip) instead of bucketize + stable argsort + gathers
            ints, reals, sc = self.engine.edge_bucket(idx, dst, gy, cnt, self.r0, self.bounds)
            if self._collective():
                send = torch.tensor(sc, dtype=torch.int64, device=dev)
                recv = self._all_to_all(send, None, None)
                rc = [int(v) for v in recv.tolist()]
                ints = self._all_to_all(ints.contiguous(), rc, sc)
                reals = self._all_to_all(reals.contiguous(), rc, sc)
            return (ints[:, 0].contiguous(), ints[:, 1].contiguous(), reals[:, 0].contiguous(), reals[:, 1].contiguous())
        valid = torch.arange(k, device=dev)[None, :] < cnt[:, None].long()
        tgt = idx[valid].long()                                                        # global target item
        src = (torch.arange(rows, device=dev) + self.r0)[:, None].expand(rows, k)[valid]
        upper = torch.tensor(self.bounds[1:], dtype=torch.int64, device=dev)
        lower = torch.tensor(self.bounds[:-1], dtype=torch.int64, device=dev)
        owner = torch.bucketize(tgt, upper, right=True)                                # bounds[o] <= tgt < bounds[o + 1]
        order = torch.argsort(owner, stable=True)
        owner = owner[order]
        ints = torch.stack([tgt[order] - lower[owner], src[order]], dim=1).to(torch.int32).contiguous()
        reals = torch.stack([dst[valid][order], gy[valid][order]], dim=1).contiguous()
        if self._collective():
            send = torch.bincount(owner, minlength=self.world).to(torch.int64)
            recv = self._all_to_all(send, None, None)
            sc, rc = [int(v) for v in send.tolist()], [int(v) for v in recv.tolist()]
            ints = self._all_to_all(ints, rc, sc)
            reals = self._all_to_all(reals, rc, sc)
        return (ints[:, 0].contiguous(), ints[:, 1].contiguous(), reals[:, 0].contiguous(), reals[:, 1].contiguous())

    def _ring_knn(self, X_shard):
        """Exact k-NN lists of this rank's rows against all items, the shards visiting one at a time.
        Step s works on the shard of rank (rank - s) mod world while the transfer for step s+1 is in flight."""
        torch, dist, e = self.torch, self.dist, self.engine
        world, rank, counts, bounds = self.world, self.rank, self.counts, self.bounds
        ring = world > 1
        e.ring_begin(world)
        mx = max(max(counts), 1)
        if ring:
            nxt_rank, prv_rank = (rank + 1) % world, (rank - 1) % world
            bufs = [torch.zeros((mx,) + tuple(X_shard.shape[1:]), dtype=X_shard.dtype, device=X_shard.device) for _ in range(2)]
            bufs[0][: X_shard.shape[0]] = X_shard
        nmax_local = torch.tensor([e.block_nmax(e.own_block())], dtype=torch.float64, device=X_shard.device)
        if ring:
            parts = [torch.zeros_like(nmax_local) for _ in range(world)]
            dist.all_gather(parts, nmax_local, group=self.group)
            nmax = [float(p.item()) for p in parts]
        else:
            nmax = [float(nmax_local.item())]
        # the block passes on the int8 images of the shards, when every rank's image allows it: each rank's measured maxima
        # (U, V, unusable) all-gathered, the ring-wide maxima handed back -- the same decision on every rank
        self.ring_i8 = False
        if hasattr(e, "ring_i8_stats"):
            # (every rank enters the all-gather below whatever its own environment or image says: a rank that may not or cannot
            # use its image -- ARROWSPACE_RING_NO_I8 set on it, no memory for the image -- reports "unusable", and all ranks
            # fall back to the bf16 passes alike; a rank that skipped the collective would leave the others waiting in it)
            try:
                mine = [0.0, 0.0, 1.0] if os.environ.get("ARROWSPACE_RING_NO_I8") else list(e.ring_i8_stats())
            except (RuntimeError, MemoryError, ValueError):
                mine = [0.0, 0.0, 1.0]
            st = torch.tensor(mine, dtype=torch.float64, device=X_shard.device)
            if ring:
                sts = [torch.zeros_like(st) for _ in range(world)]
                dist.all_gather(sts, st, group=self.group)
                st = torch.stack(sts).max(dim=0).values
            u8, v8, bad = [float(v) for v in st.tolist()]
            self.ring_i8 = e.ring_i8_set(u8, v8, bad == 0.0)

        def one_round(step_fn):
            cur = 0
            for s in range(world):
                src = (rank - s) % world
                if s == 0:
                    h, own = e.own_block(), True
                else:
                    self._sync()
                    h, own = e.open_block(bufs[cur][: counts[src]]), False
                pending = None
                if ring and s + 1 < world:
                    # the shard just worked on goes on to the next rank while it is worked on here
                    pending = self._exchange_start(bufs[cur], bufs[cur ^ 1], nxt_rank, prv_rank)
                step_fn(h, src, bounds[rank], bounds[src])
                if not own:
                    e.close_block(h)
                if pending is not None:
                    self._exchange_wait(pending)
                cur ^= 1

        lap = getattr(self, "_lap", lambda name: None)
        self.ring_symmetric = ring and hasattr(e, "knn_block_pair") and not os.environ.get("ARROWSPACE_RING_FULL")
        if self.ring_symmetric:
            self._ring_round_symmetric(X_shard, bufs, nmax)
        else:
            one_round(lambda h, b, rg, cg: e.knn_block(h, b, rg, cg))
            lap("ring_blocks")
        nflag = e.knn_merge(nmax)
        lap("ring_merge")
        if ring:
            t = torch.tensor([nflag], dtype=torch.int64, device=X_shard.device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
            anyflag = int(t.item())
        else:
            anyflag = nflag
        self.ring_flagged = nflag
        if anyflag:
            # rows not provably exact somewhere: every rank sends its shard round once more (the ring is collective);
            # ranks without flagged rows just pass the blocks on
            if ring:
                bufs[0].zero_()
                bufs[0][: X_shard.shape[0]] = X_shard
            one_round(lambda h, b, rg, cg: e.knn_block_band(h, b, rg, cg))
            e.knn_merge(nmax)
            lap("ring_round2_band")
            # rows whose band did not fit the collection buffers in some block (thousands of duplicates, or of items at one
            # distance): a third round settles them by exact evaluation of every pair -- collective as well
            nover = e.overflowed_rows() if hasattr(e, "overflowed_rows") else 0
            if ring:
                t = torch.tensor([nover], dtype=torch.int64, device=X_shard.device)
                dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
                anyover = int(t.item())
            else:
                anyover = nover
            self.ring_overflowed = nover
            if anyover:
                if ring:
                    bufs[0].zero_()
                    bufs[0][: X_shard.shape[0]] = X_shard
                one_round(lambda h, b, rg, cg: e.knn_block_exact(h, b, rg, cg))
                if nover:
                    e.knn_merge(nmax, final=True)
                lap("ring_round3_exact")
        out = e.lists()
        if ring:
            del bufs
        if hasattr(e, "ring_end"):
            e.ring_end()
        return out

    def _swap_slices(self, P, dst, src, nrows):
        """Send a block's slice home to rank dst, receive the slice of MY rows from rank src (one fp64 tensor each way)."""
        torch, dist = self.torch, self.dist
        rP = torch.empty(self.engine.slice_shape(nrows), dtype=P.dtype, device=P.device)
        ops = [dist.P2POp(dist.isend, P.contiguous(), dst, group=self.group), dist.P2POp(dist.irecv, rP, src, group=self.group)]
        for r in dist.batch_isend_irecv(ops):
            r.wait()
        return rP

    def _ring_round_symmetric(self, X_shard, bufs, nmax):
        """First round of the ring with every unordered pair of blocks computed ONCE: at step s a rank runs its rows against
        the shard of rank - s (as_knn_block_pair: the keys serve both sides), keeps its own rows' slice and sends the
        visiting rows' slice home to rank - s, receiving from rank + s the slice of its own rows against that rank's items.
        Steps 1 .. (world - 1) // 2 are whole pairs; with an even world the pair at distance world / 2 is seen from both
        ends and split: the lower rank takes the first half of the other block's column tiles, the higher rank its own rows
        of the second half.  A rank computes world / 2 + 1 blocks' worth instead of world."""
        torch, dist, e = self.torch, self.dist, self.engine
        world, rank, counts, bounds = self.world, self.rank, self.counts, self.bounds
        nxt_rank, prv_rank = (rank + 1) % world, (rank - 1) % world
        half = world // 2
        mx = max(max(counts), 1)
        # step 0: the own block, with the hop for step 1 in flight
        lap = getattr(self, "_lap", lambda name: None)
        if X_shard.is_cuda:
            torch.cuda.empty_cache()      # (the library sizes the symmetric pass's scratch by what the driver reports free; before
                                          # the hop starts: freeing memory waits for the device)
        pending = self._exchange_start(bufs[0], bufs[1], nxt_rank, prv_rank) if half >= 1 else None
        e.knn_block(e.own_block(), rank, bounds[rank], bounds[rank])
        if hasattr(torch, "cuda") and X_shard.is_cuda:
            torch.cuda.current_stream().synchronize()
        lap("ring_own_block")
        # thresholds of every item from its own block's list: what a visiting item's candidates are admitted with
        U = e.knn_thresholds(max(nmax))
        Upad = torch.full((mx,), float("inf"), dtype=torch.float32, device=U.device)
        Upad[: U.shape[0]] = U
        U_all = self._gather_fixed(Upad).reshape(world, mx)
        if pending is not None:
            self._exchange_wait(pending)
        lap("ring_thresholds_hop")
        cur = 1
        for s in range(1, half + 1):
            src = (rank - s) % world                 # whose shard is visiting, and where its slice goes home to
            dst = (rank + s) % world                 # who holds MY shard at this step
            self._sync()
            h = e.open_block(bufs[cur][: counts[src]])
            pending = self._exchange_start(bufs[cur], bufs[cur ^ 1], nxt_rank, prv_rank) if s + 1 <= half else None
            row0, row1, ct0, ct1 = 0, counts[rank], -1, -1
            if 2 * s == world:
                q = max(rank, src)                   # the higher rank's block is the one cut in halves
                tq = (counts[q] + 255) // 256 * 256 // 128
                if rank == q:
                    row0 = min(counts[q], (tq // 2) * 128)
                else:
                    ct0, ct1 = 0, tq // 2
            P = e.knn_block_pair(h, row0, row1, ct0, ct1, bounds[rank], bounds[src], U_all[src][: counts[src]], counts[src], row_thr=U)
            e.close_block(h)
            if X_shard.is_cuda:
                torch.cuda.current_stream().synchronize()
            lap("ring_pairs")
            e.fold_slice(self._swap_slices(P, src, dst, counts[rank]), nmax[dst])
            lap("ring_slice_swap_fold")
            if pending is not None:
                self._exchange_wait(pending)
            lap("ring_hop_wait")
            cur ^= 1

    def save(self, prefix):
        """One file per rank: `<prefix>.rank<r>of<world>` holds the rank's items, its lambdas and the graph."""
        self._sync()
        self.engine.save("%s.rank%dof%d" % (prefix, self.rank, self.world))

    @classmethod
    def load(cls, prefix, graph_params, dist=None, group=None, device_is_cuda=True):
        """The index `save` wrote, by the same number of ranks; no k-NN or graph work is redone."""
        import contextlib

        import torch

        self = cls()
        self.torch, self.dist, self.group = torch, dist, group
        self.world = dist.get_world_size(group) if dist is not None else 1
        self.rank = dist.get_rank(group) if dist is not None else 0
        self.engine = HipEngine(graph_params)
        self.stream = torch.cuda.Stream() if device_is_cuda else None
        ctx = torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()
        with ctx:
            off, nn = self.engine.load("%s.rank%dof%d" % (prefix, self.rank, self.world))
            rows = self.engine.n
            if self.world > 1:
                c = torch.tensor([rows], dtype=torch.int64, device=torch.device("cuda", self.engine.op.device) if device_is_cuda else "cpu")
                cs = [torch.zeros_like(c) for _ in range(self.world)]
                dist.all_gather(cs, c, group=group)
                counts = [int(v.item()) for v in cs]
            else:
                counts = [rows]
            # a replicated index saves every item in every file; a ring-built one saves the rank's rows
            self.replicated = sum(counts) != nn if self.world > 1 else False
            if self.replicated:
                counts = [b - a for a, b in zip(shard_bounds(nn, self.world)[:-1], shard_bounds(nn, self.world)[1:])]
            self.counts = counts
            self.bounds = [0]
            for v in counts:
                self.bounds.append(self.bounds[-1] + v)
            self.n = self.bounds[-1]
            self.r0, self.r1 = self.bounds[self.rank], self.bounds[self.rank + 1]
            self.scan_rows = (self.r0, self.r1) if self.replicated else (0, rows)
            self.engine.query_open()
            self._setup_library_exchange()
        return self

    def _sync(self):
        if self.stream is not None:
            self.stream.synchronize()

    def search(self, q, tau):
        """Same contract as ArrowSpace.search (src/lib.rs:132-174); every rank passes the same q."""
        import contextlib

        from . import PanicException

        e = self.engine
        if self._lib_comm:
            hits, lq, zero = e.search_staged(q, tau, *self.scan_rows)
            self.last_lambda_q = lq
            if zero:
                raise PanicException("The lambdas are zero, check the magnitude of items and eps.")
            return hits
        ctx = self.torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()
        mode = 0
        with ctx:
            if hasattr(e, "x1_usable") and e.x1_usable(tau):
                # one exchange: every rank's records and finished candidates in one all-gather, the rest redundantly on every rank
                nranks = self.world if self._collective() else 1
                e.set_mode(0)
                blocks = self._gather_fixed(e.x1_begin(q, tau, *self.scan_rows, nranks), persistent=True)
                hits, lq, zero, inexact, overflow, redo = e.x1_finish(blocks, tau, nranks)
                if redo and hasattr(e, "x1_set_coarse"):
                    # some rank's candidates did not fit -- possibly a coarse scan's wider windows: once more on the two-digit image
                    e.x1_set_coarse(False)
                    try:
                        blocks = self._gather_fixed(e.x1_begin(q, tau, *self.scan_rows, nranks), persistent=True)
                        hits, lq, zero, inexact, overflow, redo = e.x1_finish(blocks, tau, nranks)
                    finally:   # (an error in between must not leave the coarse scan switched off on this rank for good)
                        e.x1_set_coarse(True)
                mode = 0 if redo else next_mode(0, inexact, overflow)
            for _ in range(8):
                if mode is None:
                    break
                e.set_mode(mode)
                e.query_scan(q, *self.scan_rows)
                knn_all = self._gather_fixed(e.knn_local, persistent=True)
                e.query_lambda(knn_all)
                e.query_score(tau)
                hits_all = self._gather_fixed(e.hits_local, persistent=True)
                hits, lq, zero, inexact, overflow = e.query_finish(hits_all)
                mode = next_mode(mode, inexact, overflow)
                if mode is None:
                    break
            else:   # next_mode is strictly increasing: unreachable, and never a silently wrong answer
                raise RuntimeError("sharded search did not settle on an exact answer")
        self.last_lambda_q = lq
        if zero:
            raise PanicException("The lambdas are zero, check the magnitude of items and eps.")
        return hits

    def search_batch(self, Q, tau):
        """B queries [B, D] -> list of B hit lists: 32 query slots per pass over every rank's rows, the two record
        exchanges of a pass shared by its slots.  A query the batched fast path cannot prove exact is rerun through
        search() -- every rank sees the same merged flags, so every rank reruns the same ones."""
        import contextlib

        from . import PanicException

        e = self.engine
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        if Q.ndim != 2:
            raise TypeError("items must be a 2-D float64 array")
        if not hasattr(e, "query_scan_batch"):
            return [self.search(np.ascontiguousarray(q), tau) for q in Q]
        nranks = self.world if self._collective() else 1
        ctx = self.torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()
        out, zero_any = [], False
        with ctx:
            if not getattr(self, "_batch_cap", 0):
                self._batch_cap = e.batch_open()
            cap = self._batch_cap
            for i0 in range(0, Q.shape[0], cap):
                chunk = Q[i0 : i0 + cap]
                e.query_scan_batch(chunk, *self.scan_rows)
                knn_all = self._gather_fixed(e.knn_local_b, persistent=True)
                e.query_lambda_batch(knn_all, nranks)
                e.query_score_batch(tau)
                hits_all = self._gather_fixed(e.hits_local_b, persistent=True)
                for b, (hits, lq, zero) in enumerate(e.query_finish_batch(hits_all, nranks, chunk.shape[0])):
                    if hits is None:
                        try:
                            hits = self.search(np.ascontiguousarray(chunk[b]), tau)
                        except PanicException:
                            zero, hits = True, []
                    zero_any = zero_any or zero
                    out.append(hits)
        if zero_any:
            raise PanicException("The lambdas are zero, check the magnitude of items and eps.")
        return out

    def lambdas(self):
        """lambdas of ALL items, in item order (ring build: every rank holds its own rows' -- gathered here)."""
        lam = self.engine.lambdas()
        if self.replicated or not self._collective():
            return lam
        torch = self.torch
        dev = self.engine.knn_local.device
        t = torch.from_numpy(np.ascontiguousarray(lam[: self.counts[self.rank]])).to(dev)
        return self._gather_rows(t, self.counts).cpu().numpy()

    def degrees(self):
        """Weighted degrees of ALL items, in item order (a collective on a row-sharded graph: every rank holds its rows')."""
        deg = self.engine.degrees()
        if self.replicated or not self._collective() or len(deg) == self.n:
            return deg
        torch = self.torch
        dev = self.engine.knn_local.device
        t = torch.from_numpy(np.ascontiguousarray(deg[: self.counts[self.rank]])).to(dev)
        return self._gather_rows(t, self.counts).cpu().numpy()

    def last_scan_us(self):
        return self.engine.scan_us(self.engine.qs if self._lib_comm else None)

    def last_scan_operand(self):
        """What this rank's last single-query scan read: "fp32" items, their "int8" two-digit image or "int8-high" (coarse)."""
        e = self.engine
        q = e.qs if self._lib_comm else e.q
        return {0: "fp32", 1: "int8", 2: "int8-high"}.get(int(e.L.as_query_scan_int8(q)), "fp32")

    @property
    def last_scan_bits(self):
        """Width of the coarse operand this rank's last single-query scan read: 4 (nibble tiles) or 8."""
        e = self.engine
        q = e.qs if self._lib_comm else e.q
        return int(e.L.as_query_scan_bits(q))

    def build_stats(self):
        return getattr(self.engine, "stats", lambda: {})()

    def close(self):
        if self.engine is not None:
            self.engine.close()
            self.engine = None


class HostStagedIndex(ShardedIndex):
    """ShardedIndex whose every exchange step is staged through host memory (torch.distributed backend "gloo"): the
    form for ranks that SHARE one GPU -- RCCL wants one device per rank -- i.e. the one-GPU rehearsal of an N-rank job
    (bench.py --gpus N on a box with fewer devices, the multi-rank tests of tests/test_gpu_*.py).  Same host logic,
    same kernels, same results; only the transport differs."""

    library_exchange = False      # (gloo ranks sharing a GPU: no RCCL communicator)

    @classmethod
    def build(cls, graph_params, X_shard, dist=None, *args, **kwargs):
        # The ranks share ONE card: the library sizes its scratch (the symmetric pass's transposed buffers: 8 KB per item) by
        # the memory it finds free -- found free by every rank at the same moment.  Each rank plans with its share.
        # (set around THIS build only: a later build in the process measures again -- the card is fuller by then -- and a plain
        # ShardedIndex / ArrowSpace build is not handed a share meant for ranks that shared a card)
        group = kwargs.get("group", args[0] if args else None)
        mine = dist is not None and getattr(X_shard, "is_cuda", False) and "ARROWSPACE_SYM_FREE_GB" not in os.environ
        if mine:
            import torch
            free, _ = torch.cuda.mem_get_info(X_shard.device)
            os.environ["ARROWSPACE_SYM_FREE_GB"] = "%.1f" % (0.8 * free / 1e9 / max(dist.get_world_size(group), 1))
        try:
            return super().build(graph_params, X_shard, dist, *args, **kwargs)
        finally:
            if mine:
                os.environ.pop("ARROWSPACE_SYM_FREE_GB", None)


    def _gather_rows(self, t, counts):
        self.torch.cuda.synchronize()
        return super()._gather_rows(t.cpu(), counts).cuda()

    def _gather_fixed(self, t, persistent=False):
        torch = self.torch
        torch.cuda.synchronize()
        if not (persistent and t.is_cuda and self._collective()):
            return super()._gather_fixed(t.cpu()).cuda()
        # the engine's record tensors, gathered for every query: pinned host buffers and the device result are made once
        key = ("host", t.data_ptr(), tuple(t.shape), t.dtype)
        bufs = self._gbuf.get(key)
        if bufs is None:
            hs = torch.empty(tuple(t.shape), dtype=t.dtype).pin_memory()
            hr = torch.empty((self.world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype).pin_memory()
            out = torch.empty(tuple(hr.shape), dtype=t.dtype, device=t.device)
            bufs = self._gbuf[key] = (hs, hr, out)
        hs, hr, out = bufs
        hs.copy_(t)
        self.dist.all_gather_into_tensor(hr, hs, group=self.group)
        out.copy_(hr)
        torch.cuda.synchronize()
        return out

    def _swap_slices(self, P, dst, src, nrows):                  # the symmetric ring's slices
        self.torch.cuda.synchronize()
        return super()._swap_slices(P.cpu(), dst, src, nrows).cuda()

    def _all_to_all(self, t, recv_counts, send_counts):           # the edge exchange of the sharded graph stage
        self.torch.cuda.synchronize()
        return super()._all_to_all(t.cpu(), recv_counts, send_counts).cuda()

    def _exchange_start(self, send, recv, nxt_rank, prv_rank):   # the ring hop
        torch = self.torch
        torch.cuda.synchronize()
        hs, hr = send.cpu(), torch.empty(recv.shape, dtype=recv.dtype)
        return (super()._exchange_start(hs, hr, nxt_rank, prv_rank), hr, recv, hs)

    def _exchange_wait(self, pending):
        reqs, hr, recv, _ = pending
        super()._exchange_wait(reqs)
        recv.copy_(hr)
        self.torch.cuda.synchronize()
