// Fixed-point diffusion search (section 5.23): conjugate gradients on (I - alpha S) f = (1 - alpha) y over the
// item graph, S and y those of S19 (as_diffuse.hip), per column of a chunk and independent of every other column.  Four vectors
// x, r, p, q are [N][C] doubles, item-major, C = 1, 16 or 64.  The only reduction is S20's dot: segments of 64 rows summed in row
// order, then a halving tree over the segments -- the apply and update kernels leave the segment partials of p.q and r.r in the
// same pass that writes q and r, the reduce kernel runs the tree and forms the column's scalars (a, g, rho, the stopping tests)
// on the device.  A column that has stopped (converged, or p.q not > 0) is frozen: every kernel tests its state before it writes
// that column's x, r, p or scalars.  The host reads the states once per iteration through pinned memory and ends the chunk when no
// column is live; it steers no arithmetic.  Every product, sum, difference and quotient is rounded once (contract off, plain /).
// Entry points: as_api.hip (as_search_diffuse_solve, as_search_diffuse_solve_batch, as_score_diffuse_solve_batch,
// as_diffuse_solve_seeds).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>

#include "as_diffuse.hpp"

// S20 rounds every operation once: no multiply of this file may be fused with the add or subtract behind it
#pragma clang fp contract(off)

namespace as {

constexpr int SOL_SEG = 64;              // rows of a segment of S20's dot
constexpr int SOL_REDUCE_THREADS = 1024;
enum { SOL_LIVE = 0, SOL_CONVERGED = 1, SOL_BREAKDOWN = 2 };
enum { SOL_RED_INIT = 0, SOL_RED_PQ = 1, SOL_RED_RR = 2 };

// the scalars of the columns of a chunk, on the device and (copied once per iteration) in pinned memory
struct SolveScalars {
    double rho[DIF_SOLVE_COLS], bb[DIF_SOLVE_COLS], theta[DIF_SOLVE_COLS], a[DIF_SOLVE_COLS], g[DIF_SOLVE_COLS];
    int32_t state[DIF_SOLVE_COLS], iters[DIF_SOLVE_COLS];
};

struct SolveArgs {
    const int64_t* indptr;    // [n + 1]
    const int32_t* indices;   // [nnz]
    const double* lap;        // [nnz]: S_e = -lap[e]
    double* x;                // [n][C] each
    double* r;
    double* p;
    double* q;
    double* part;             // [ceil(n / 64)][C]: the segment partials of the dot in flight
    SolveScalars* sc;
    int64_t n;
    double alpha;
    int tile;                 // the C = 1 apply kernel: edges per LDS tile
    int dot_only;             // the update kernel at the start: the partials of r.r, nothing written to x or r
};

// the 64 products of each of a block's four segments, chained in row order by one lane per segment (C = 1)
__device__ __forceinline__ void solve_chain_segments(const double* prod, int64_t first, int64_t n, int64_t group, double* part) {
    const int tid = threadIdx.x;
    if (tid < DIF_THREADS / SOL_SEG && first + (int64_t)tid * SOL_SEG < n) {
        const int64_t left = n - (first + (int64_t)tid * SOL_SEG);
        const int rows = left < SOL_SEG ? (int)left : SOL_SEG;
        double sigma = 0.0;
        for (int j = 0; j < rows; ++j) sigma = sigma + prod[tid * SOL_SEG + j];
        part[group * (DIF_THREADS / SOL_SEG) + tid] = sigma;
    }
}

// q = p - alpha S p and the segment partials of p.q.
// CT = 1: a block owns groups of 256 rows (four segments); the edges of a group stream through LDS as in diffuse_step1_kernel, one
// lane per row keeps the row's sum in CSR order; then the products p_i q_i go to LDS and one lane per segment chains them.
// CT = 16, 64: lanes own columns; a wave owns 64 / CT segments (one per group of CT lanes) and walks a segment's rows in ascending
// order, the row sum as in diffuse_step_cols_kernel, sigma in a register.
template <int CT>
__global__ __launch_bounds__(DIF_THREADS) void solve_apply_kernel(SolveArgs a) {
    if constexpr (CT == 1) {
        extern __shared__ double sol_prod[];
        __shared__ double sol_pq[DIF_THREADS];
        if (a.sc->state[0] != SOL_LIVE) return;   // (the whole block)
        const int tid = threadIdx.x, T = a.tile;
        const int64_t groups = (a.n + DIF_THREADS - 1) / DIF_THREADS;
        for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
            const int64_t first = g * DIF_THREADS, last = first + DIF_THREADS < a.n ? first + DIF_THREADS : a.n;
            const int64_t row = first + tid;
            const bool live = row < last;
            const int64_t rs = live ? a.indptr[row] : 0, re = live ? a.indptr[row + 1] : 0;
            const int64_t e0 = a.indptr[first], e1 = a.indptr[last];
            double acc = 0.0;
            for (int64_t s0 = e0; s0 < e1; s0 += T) {
                const int64_t s1 = s0 + T < e1 ? s0 + T : e1;
                for (int64_t e = s0 + tid; e < s1; e += DIF_THREADS) sol_prod[e - s0] = -a.lap[e] * a.p[a.indices[e]];
                __syncthreads();
                const int64_t lo = rs > s0 ? rs : s0, hi = re < s1 ? re : s1;
                for (int64_t e = lo; e < hi; ++e) acc = acc + sol_prod[e - s0];
                __syncthreads();   // the tile is read before the next one is written
            }
            double pq = 0.0;
            if (live) {
                const double pv = a.p[row];
                const double qv = pv - a.alpha * acc;
                a.q[row] = qv;
                pq = pv * qv;
            }
            sol_pq[tid] = pq;
            __syncthreads();
            solve_chain_segments(sol_pq, first, a.n, g, a.part);
            __syncthreads();   // the products are read before the next group writes them
        }
    } else {
        constexpr int SPW = 64 / CT;
        const int lane = threadIdx.x & 63, c = lane % CT, sub = lane / CT;
        if (a.sc->state[c] != SOL_LIVE) return;   // a frozen column's lanes leave: nothing below spans lanes
        const int64_t nseg = (a.n + SOL_SEG - 1) / SOL_SEG;
        const int64_t waves = (int64_t)gridDim.x * (DIF_THREADS / 64);
        const double* __restrict__ f = a.p + c;
        for (int64_t s0 = ((int64_t)blockIdx.x * (DIF_THREADS / 64) + (threadIdx.x >> 6)) * SPW; s0 < nseg; s0 += waves * SPW) {
            const int64_t s = s0 + sub;
            if (s >= nseg) continue;
            const int64_t first = s * SOL_SEG, last = first + SOL_SEG < a.n ? first + SOL_SEG : a.n;
            double sigma = 0.0;
            for (int64_t row = first; row < last; ++row) {
                const int64_t rs = a.indptr[row], re = a.indptr[row + 1];
                double acc = 0.0;
                int64_t e = rs;
                for (; e + 4 <= re; e += 4) {
                    const double w0 = -a.lap[e], w1 = -a.lap[e + 1], w2 = -a.lap[e + 2], w3 = -a.lap[e + 3];
                    const double v0 = f[(int64_t)a.indices[e] * CT], v1 = f[(int64_t)a.indices[e + 1] * CT];
                    const double v2 = f[(int64_t)a.indices[e + 2] * CT], v3 = f[(int64_t)a.indices[e + 3] * CT];
                    acc = acc + w0 * v0;
                    acc = acc + w1 * v1;
                    acc = acc + w2 * v2;
                    acc = acc + w3 * v3;
                }
                for (; e < re; ++e) acc = acc + (-a.lap[e] * f[(int64_t)a.indices[e] * CT]);
                const double pv = f[row * CT];
                const double qv = pv - a.alpha * acc;
                a.q[row * CT + c] = qv;
                sigma = sigma + pv * qv;
            }
            a.part[s * CT + c] = sigma;
        }
    }
}

// x += a p, r -= a q and the segment partials of r.r, one pass, the wave-to-segment mapping of the apply kernel.  dot_only: the
// partials of r.r alone (rho at the start).
template <int CT>
__global__ __launch_bounds__(DIF_THREADS) void solve_update_kernel(SolveArgs a) {
    if constexpr (CT == 1) {
        __shared__ double sol_rr[DIF_THREADS];
        if (a.sc->state[0] != SOL_LIVE) return;
        const int tid = threadIdx.x;
        const double av = a.sc->a[0];
        const int64_t groups = (a.n + DIF_THREADS - 1) / DIF_THREADS;
        for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
            const int64_t first = g * DIF_THREADS, row = first + tid;
            double rr = 0.0;
            if (row < a.n) {
                double rv = a.r[row];
                if (!a.dot_only) {
                    a.x[row] = a.x[row] + av * a.p[row];
                    rv = rv - av * a.q[row];
                    a.r[row] = rv;
                }
                rr = rv * rv;
            }
            sol_rr[tid] = rr;
            __syncthreads();
            solve_chain_segments(sol_rr, first, a.n, g, a.part);
            __syncthreads();
        }
    } else {
        constexpr int SPW = 64 / CT;
        const int lane = threadIdx.x & 63, c = lane % CT, sub = lane / CT;
        if (a.sc->state[c] != SOL_LIVE) return;
        const double av = a.sc->a[c];
        const int64_t nseg = (a.n + SOL_SEG - 1) / SOL_SEG;
        const int64_t waves = (int64_t)gridDim.x * (DIF_THREADS / 64);
        for (int64_t s0 = ((int64_t)blockIdx.x * (DIF_THREADS / 64) + (threadIdx.x >> 6)) * SPW; s0 < nseg; s0 += waves * SPW) {
            const int64_t s = s0 + sub;
            if (s >= nseg) continue;
            const int64_t first = s * SOL_SEG, last = first + SOL_SEG < a.n ? first + SOL_SEG : a.n;
            double sigma = 0.0;
#pragma unroll 4
            for (int64_t row = first; row < last; ++row) {
                const int64_t i = row * CT + c;
                double rv = a.r[i];
                if (!a.dot_only) {
                    a.x[i] = a.x[i] + av * a.p[i];
                    rv = rv - av * a.q[i];
                    a.r[i] = rv;
                }
                sigma = sigma + rv * rv;
            }
            a.part[s * CT + c] = sigma;
        }
    }
}

// p = r + g p over the live columns, one thread per cell
__global__ __launch_bounds__(DIF_THREADS) void solve_direction_kernel(SolveArgs a, int C) {
    const int64_t cells = a.n * C;
    for (int64_t i = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; i < cells; i += (int64_t)gridDim.x * DIF_THREADS) {
        const int c = (int)(i & (C - 1));
        if (a.sc->state[c] != SOL_LIVE) continue;
        a.p[i] = a.r[i] + a.sc->g[c] * a.p[i];
    }
}

// One block per column: S20's halving tree over the column's nseg partials (in place; an entry past nseg counts as +0.0), then the
// column's scalars.  INIT: rho = bb = dot, theta = fl(fl(tol tol) bb), converged at once if bb = 0.  PQ: breakdown unless dot > 0,
// else a = fl(rho / dot).  RR: iterations + 1; converged if dot <= theta, else g = fl(dot / rho); rho = dot.
__global__ __launch_bounds__(SOL_REDUCE_THREADS) void solve_reduce_kernel(double* part, int C, int64_t nseg, SolveScalars* sc, int mode, double tol) {
    const int c = blockIdx.x;
    if (sc->state[c] != SOL_LIVE) return;   // (the whole block)
    int64_t P = 1;
    while (P < nseg) P <<= 1;
    for (int64_t h = P >> 1; h >= 1; h >>= 1) {
        const int64_t top = h < nseg ? h : nseg;
        for (int64_t j = threadIdx.x; j < top; j += SOL_REDUCE_THREADS) {
            const double hi = j + h < nseg ? part[(j + h) * C + c] : 0.0;
            part[j * C + c] = part[j * C + c] + hi;
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double t = part[c];
    if (mode == SOL_RED_INIT) {
        sc->rho[c] = t;
        sc->bb[c] = t;
        sc->theta[c] = (tol * tol) * t;
        if (t == 0.0) sc->state[c] = SOL_CONVERGED;
    } else if (mode == SOL_RED_PQ) {
        if (!(t > 0.0)) sc->state[c] = SOL_BREAKDOWN;
        else sc->a[c] = sc->rho[c] / t;
    } else {
        sc->iters[c] = sc->iters[c] + 1;
        if (t <= sc->theta[c]) sc->state[c] = SOL_CONVERGED;
        else sc->g[c] = t / sc->rho[c];
        sc->rho[c] = t;
    }
}

// ------------------------------------------------------------------ host side
static std::atomic<int> g_solve_mib{DIF_SOLVE_MIB_DEFAULT};
void set_diffuse_solve_mib(int v) { g_solve_mib.store(v > 0 ? v : DIF_SOLVE_MIB_DEFAULT, std::memory_order_relaxed); }
double diffuse_solve_kernel_us(const DiffuseWork* w, int part) {
    if (!w || part < 0 || part > 5) return 0.0;
    return part == 0 ? w->solve_us : w->solve_part_us[part - 1];
}

static unsigned solve_grid(const DiffuseWork* w, int64_t blocks) {
    return diffuse_grid(std::min<int64_t>(blocks, (int64_t)w->cus * DIF_BLOCKS_PER_CU));
}

static void solve_apply_launch(const DiffuseWork* w, const SolveArgs& a, int C) {
    const int64_t nseg = (a.n + SOL_SEG - 1) / SOL_SEG;
    if (C == 1) {
        const unsigned grid = solve_grid(w, (a.n + DIF_THREADS - 1) / DIF_THREADS);
        hipLaunchKernelGGL(solve_apply_kernel<1>, dim3(grid), dim3(DIF_THREADS), sizeof(double) * (size_t)a.tile, w->stream, a);
        return;
    }
    const int64_t per_block = (int64_t)(DIF_THREADS / 64) * (64 / C);   // segments of a block and trip
    const unsigned grid = solve_grid(w, (nseg + per_block - 1) / per_block);
    if (C == 16) hipLaunchKernelGGL(solve_apply_kernel<16>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
    else hipLaunchKernelGGL(solve_apply_kernel<64>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
}

static void solve_update_launch(const DiffuseWork* w, const SolveArgs& a, int C) {
    const int64_t nseg = (a.n + SOL_SEG - 1) / SOL_SEG;
    if (C == 1) {
        const unsigned grid = solve_grid(w, (a.n + DIF_THREADS - 1) / DIF_THREADS);
        hipLaunchKernelGGL(solve_update_kernel<1>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
        return;
    }
    const int64_t per_block = (int64_t)(DIF_THREADS / 64) * (64 / C);
    const unsigned grid = solve_grid(w, (nseg + per_block - 1) / per_block);
    if (C == 16) hipLaunchKernelGGL(solve_update_kernel<16>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
    else hipLaunchKernelGGL(solve_update_kernel<64>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
}

as_status diffuse_solve_chunks(const as_space* sp, const as_graph* gr, const DiffuseCall& c, int64_t* counts) {
    const int64_t n = gr->n;
    DiffuseFrame fr;
    AS_TRY(diffuse_frame(sp, gr, c, &fr));
    if (!fr.w) return AS_OK;
    DiffuseWork* w = fr.w;
    const bool timing = diffuse_timing();
    const int cols_cap = diffuse_cols_cap();
    const int64_t budget = (int64_t)g_solve_mib.load(std::memory_order_relaxed) << 20;
    const double om = 1.0 - c.alpha;
    const int64_t nseg = (n + SOL_SEG - 1) / SOL_SEG;
    w->solve_us = 0.0;
    for (double& v : w->solve_part_us) v = 0.0;
    dev_events<6> pe;   // timing: the five launches of one sampled iteration (the second of a chunk, or its only one)
    if (timing) AS_HIP(pe.create());
    AS_TRY(reserve_or_err(w->scal_d, sizeof(SolveScalars), "diffuse solve scalars"));
    AS_TRY(reserve_or_err(w->scal_h, sizeof(SolveScalars), "diffuse solve pinned scalars"));
    SolveScalars* const sd = (SolveScalars*)(char*)w->scal_d;
    SolveScalars* const sh = (SolveScalars*)(char*)w->scal_h;
    const int64_t nq = (int64_t)fr.q.size();
    for (int64_t i0 = 0; i0 < nq;) {
        const int C = diffuse_chunk_cols(nq - i0, n, cols_cap, budget, 4);
        const int64_t nc = std::min<int64_t>(C, nq - i0);
        for (int s = 0; s < 2; ++s) {
            AS_TRY(reserve_or_err(w->f[s], n * C, "diffuse f buffers"));
            AS_TRY(reserve_or_err(w->sv[s], n * C, "diffuse solve vectors"));
        }
        AS_TRY(reserve_or_err(w->part, nseg * C, "diffuse solve partials"));
        DiffuseSeeds seeds;
        AS_TRY(diffuse_seed_table(fr, c, i0, nc, &seeds));
        SolveArgs a;
        a.indptr = gr->indptr; a.indices = gr->indices; a.lap = gr->lap;
        a.x = w->f[0]; a.r = w->f[1]; a.p = w->sv[0]; a.q = w->sv[1]; a.part = w->part; a.sc = sd;
        a.n = n; a.alpha = c.alpha; a.tile = diffuse_tile_edges(); a.dot_only = 0;
        // x = 0, r = p = b = fl(om y): the seed kernel's add mode on zeroed buffers.  The columns past nc start frozen.
        const size_t bytes = sizeof(double) * (size_t)(n * C);
        AS_HIP(hipMemsetAsync(a.x, 0, bytes, w->stream));
        AS_HIP(hipMemsetAsync(a.r, 0, bytes, w->stream));
        AS_HIP(hipMemsetAsync(a.p, 0, bytes, w->stream));
        diffuse_seed_launch(w, seeds, a.r, C, om, 0);
        diffuse_seed_launch(w, seeds, a.p, C, om, 0);
        std::memset(sh, 0, sizeof(SolveScalars));
        for (int t = 0; t < DIF_SOLVE_COLS; ++t) sh->state[t] = t < nc ? SOL_LIVE : SOL_CONVERGED;
        AS_HIP(hipMemcpyAsync(sd, sh, sizeof(SolveScalars), hipMemcpyHostToDevice, w->stream));
        SolveArgs a0 = a;
        a0.dot_only = 1;
        solve_update_launch(w, a0, C);
        hipLaunchKernelGGL(solve_reduce_kernel, dim3((unsigned)nc), dim3(SOL_REDUCE_THREADS), 0, w->stream, a.part, C, nseg, sd, (int)SOL_RED_INIT, c.tol);
        AS_HIP(hipGetLastError());
        AS_HIP(hipMemcpyAsync(sh, sd, sizeof(SolveScalars), hipMemcpyDeviceToHost, w->stream));
        AS_HIP(hipStreamSynchronize(w->stream));
        int64_t waits = 1, k = 0;
        auto any_live = [&]() {
            for (int64_t t = 0; t < nc; ++t)
                if (sh->state[t] == SOL_LIVE) return true;
            return false;
        };
        bool live = any_live();
        if (timing) AS_HIP(hipEventRecord(w->ev.e[0], w->stream));
        const unsigned dgrid = solve_grid(w, (n * C + DIF_THREADS - 1) / DIF_THREADS);
        while (live && k < c.max_iters) {
            ++k;
            const bool sample = timing && (k == 2 || (k == 1 && c.max_iters == 1));
            if (sample) AS_HIP(hipEventRecord(pe.e[0], w->stream));
            solve_apply_launch(w, a, C);
            if (sample) AS_HIP(hipEventRecord(pe.e[1], w->stream));
            hipLaunchKernelGGL(solve_reduce_kernel, dim3((unsigned)nc), dim3(SOL_REDUCE_THREADS), 0, w->stream, a.part, C, nseg, sd, (int)SOL_RED_PQ, c.tol);
            if (sample) AS_HIP(hipEventRecord(pe.e[2], w->stream));
            solve_update_launch(w, a, C);
            if (sample) AS_HIP(hipEventRecord(pe.e[3], w->stream));
            hipLaunchKernelGGL(solve_reduce_kernel, dim3((unsigned)nc), dim3(SOL_REDUCE_THREADS), 0, w->stream, a.part, C, nseg, sd, (int)SOL_RED_RR, c.tol);
            if (sample) AS_HIP(hipEventRecord(pe.e[4], w->stream));
            AS_HIP(hipMemcpyAsync(sh, sd, sizeof(SolveScalars), hipMemcpyDeviceToHost, w->stream));
            // the next direction runs behind the copy while the host waits: it tests the states itself
            if (k < c.max_iters) hipLaunchKernelGGL(solve_direction_kernel, dim3(dgrid), dim3(DIF_THREADS), 0, w->stream, a, C);
            if (sample) AS_HIP(hipEventRecord(pe.e[5], w->stream));
            AS_HIP(hipGetLastError());
            AS_HIP(hipStreamSynchronize(w->stream));
            ++waits;
            live = any_live();
            for (int t = 0; sample && t < 5; ++t) {
                float ms = 0.0f;
                AS_HIP(hipEventElapsedTime(&ms, pe.e[t], pe.e[t + 1]));
                w->solve_part_us[t] += (double)ms * 1e3;   // (the fifth holds the copy of the scalars too)
            }
        }
        if (timing) AS_HIP(hipEventRecord(w->ev.e[1], w->stream));
        for (int64_t t = 0; t < nc; ++t) {
            const int64_t i = fr.q[i0 + t];
            if (c.out_iters) c.out_iters[i] = sh->iters[t];
            if (c.out_residual) c.out_residual[i] = sh->bb[t] == 0.0 ? 0.0 : std::sqrt(sh->rho[t] / sh->bb[t]);
            if (c.out_state) c.out_state[i] = sh->state[t] == SOL_LIVE ? 0 : sh->state[t];
        }
        counts[0] += 1;
        counts[1] += k;
        counts[2] += waits;
        counts[3] += seeds.ns;
        AS_TRY(diffuse_emit(fr, c, i0, nc, C, a.x, timing, &w->solve_us));
        i0 += nc;
    }
    return AS_OK;
}

}  // namespace as
