// Fused multi-query search: ONE answer to J query vectors -- F(i) = the weighted sum, or the largest
// weighted term, of the J S11 scores of item i.  The scores come from the batched filtered forms' score kernel (as_subset.hip),
// unchanged, a chunk of queries at a time; this file folds each chunk's [nb][ld] block into one accumulator [m] that stays on the
// device (fused_accumulate_kernel) and carries over the chunks, so J is not bound by the chunk size.  The order over j inside a
// position is sequential and ascending: that order is the specification (S13), the numpy loop reproduces the bits.
// Entry points: as_api.hip (as_search_fused, as_score_fused, as_fused_counters, as_fused_kernel_us).
// The batched form (S15, section 5.18): B needs of J_b vectors each in one call.  The vectors of all needs are ONE flattened list
// of rows for the score kernel; fused_accumulate_batch_kernel folds each chunk of rows segment by segment into one accumulator
// row per need ([G][m], G needs at a time).  Entry points: as_search_fused_batch, as_score_fused_batch, as_fused_batch_counters,
// as_fused_batch_kernel_us.
#include <algorithm>
#include <atomic>
#include <new>

#include "as_common.hpp"
#include "as_fused_step.hpp"   // fused_step: one step of S13, never contracted into an FMA

namespace as {

// a pair of scores of one row: rows start on an 8-byte boundary only (ld may be odd), so the type promises no more than that;
// the load is still one 16-byte instruction
typedef double f64x2_a8 __attribute__((ext_vector_type(2), aligned(8)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int FA_THREADS = 256;
constexpr int FA_ROWS = 8;             // rows whose loads are in flight together
constexpr int FA_BLOCKS_PER_CU = 8;    // the grid: that many blocks per CU at most, the rest is the grid-stride loop

// acc[i] <- the fold of rows 0 .. nb - 1 of scores ([nb][ld]) at position i < m onto acc[i], rows ascending; a row whose flag is 0
// is skipped.  fresh: the accumulator holds nothing yet -- the first served row of the chunk initialises it (no memset, no 0 + t).
// A thread owns a pair of neighbouring positions (16-byte loads and stores; the accumulator is 16-byte aligned) for all rows, so no
// two threads meet in a position and the stores are plain; an odd m leaves one single position to the thread behind the last pair.
template <int MODE>
__global__ __launch_bounds__(FA_THREADS) void fused_accumulate_kernel(const double* __restrict__ scores, int64_t ld, int64_t m, int nb,
                                                                      const double* __restrict__ wts, const int32_t* __restrict__ flags,
                                                                      double* __restrict__ acc, int fresh) {
    const int64_t pairs = m >> 1, units = pairs + (m & 1);
    for (int64_t u = (int64_t)blockIdx.x * FA_THREADS + threadIdx.x; u < units; u += (int64_t)gridDim.x * FA_THREADS) {
        const bool pair = u < pairs;
        const int64_t i = 2 * u;   // (the single position of an odd m: i == m - 1)
        bool have = fresh == 0;
        double f0 = 0.0, f1 = 0.0;
        if (have) {
            if (pair) {
                const f64x2 a = *(const f64x2*)(acc + i);
                f0 = a[0];
                f1 = a[1];
            } else {
                f0 = acc[i];
            }
        }
        for (int j0 = 0; j0 < nb; j0 += FA_ROWS) {
            double s0[FA_ROWS], s1[FA_ROWS];
#pragma unroll
            for (int r = 0; r < FA_ROWS; ++r) {
                s0[r] = 0.0;
                s1[r] = 0.0;
                if (j0 + r < nb) {
                    const double* p = scores + (int64_t)(j0 + r) * ld + i;
                    if (pair) {
                        const f64x2_a8 x = *(const f64x2_a8*)p;
                        s0[r] = x[0];
                        s1[r] = x[1];
                    } else {
                        s0[r] = *p;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < FA_ROWS; ++r) {
                if (j0 + r < nb && flags[j0 + r]) {
                    const double wj = wts[j0 + r];
                    f0 = fused_step<MODE>(f0, wj, s0[r], have);
                    f1 = fused_step<MODE>(f1, wj, s1[r], have);
                    have = true;
                }
            }
        }
        if (!have) continue;   // (no served row so far: the host does not launch such a chunk)
        if (pair) {
            f64x2 o;
            o[0] = f0;
            o[1] = f1;
            *(f64x2*)(acc + i) = o;
        } else {
            acc[i] = f0;
        }
    }
}

// The segmented fold of the batched form.  The chunk scores ([nb][ld]) holds the flattened rows r0 .. r0 + nb - 1 of the call; need
// y = need0 + blockIdx.y owns rows offs[y] .. offs[y + 1] - 1 of them, cut by the chunk's edges, and the accumulator row
// acc + (y - gneed0) * m.  first[y] / last[y]: the flattened index of the need's first / last served row (-1: none) -- the need's
// accumulator holds something iff its first served row lies before the rows taken here, so no launch has to be told; a need
// without a served row at or before / at or behind this chunk leaves at once (block-uniform: y is).  Inside a need the kernel is
// fused_accumulate_kernel: a thread owns a pair of neighbouring positions for all the need's rows, FA_ROWS loads in flight,
// rows ascending, plain 16-byte stores.  An accumulator row starts on an 8-byte boundary only (m may be odd): f64x2_a8.
template <int MODE>
__global__ __launch_bounds__(FA_THREADS) void fused_accumulate_batch_kernel(const double* __restrict__ scores, int64_t ld, int64_t m, int64_t r0,
                                                                            int nb, int64_t need0, int64_t gneed0,
                                                                            const int64_t* __restrict__ offs, const int64_t* __restrict__ first,
                                                                            const int64_t* __restrict__ last, const double* __restrict__ wts,
                                                                            const int32_t* __restrict__ flags, double* __restrict__ acc) {
    const int64_t need = need0 + blockIdx.y;
    const int64_t o0 = offs[need], o1 = offs[need + 1];
    const int64_t lo = o0 > r0 ? o0 : r0, hi = o1 < r0 + nb ? o1 : r0 + nb;
    const int64_t fs = first[need];
    if (fs < 0 || fs >= hi || last[need] < lo) return;
    const bool carried = fs < lo;
    const int n = (int)(hi - lo);
    const double* __restrict__ rows = scores + (lo - r0) * ld;
    const double* __restrict__ w = wts + lo;
    const int32_t* __restrict__ fl = flags + lo;
    double* __restrict__ a = acc + (need - gneed0) * m;
    const int64_t pairs = m >> 1, units = pairs + (m & 1);
    for (int64_t u = (int64_t)blockIdx.x * FA_THREADS + threadIdx.x; u < units; u += (int64_t)gridDim.x * FA_THREADS) {
        const bool pair = u < pairs;
        const int64_t i = 2 * u;   // (the single position of an odd m: i == m - 1)
        bool have = carried;
        double f0 = 0.0, f1 = 0.0;
        if (have) {
            if (pair) {
                const f64x2_a8 x = *(const f64x2_a8*)(a + i);
                f0 = x[0];
                f1 = x[1];
            } else {
                f0 = a[i];
            }
        }
        bool touched = false;
        for (int j0 = 0; j0 < n; j0 += FA_ROWS) {
            double s0[FA_ROWS], s1[FA_ROWS];
#pragma unroll
            for (int r = 0; r < FA_ROWS; ++r) {
                s0[r] = 0.0;
                s1[r] = 0.0;
                if (j0 + r < n) {
                    const double* p = rows + (int64_t)(j0 + r) * ld + i;
                    if (pair) {
                        const f64x2_a8 x = *(const f64x2_a8*)p;
                        s0[r] = x[0];
                        s1[r] = x[1];
                    } else {
                        s0[r] = *p;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < FA_ROWS; ++r) {
                if (j0 + r < n && fl[j0 + r]) {
                    const double wj = w[j0 + r];
                    f0 = fused_step<MODE>(f0, wj, s0[r], have);
                    f1 = fused_step<MODE>(f1, wj, s1[r], have);
                    have = true;
                    touched = true;
                }
            }
        }
        if (!touched) continue;   // (served rows before and behind this chunk, none inside: the accumulator stays as it is)
        if (pair) {
            f64x2_a8 o;
            o[0] = f0;
            o[1] = f1;
            *(f64x2_a8*)(a + i) = o;
        } else {
            a[i] = f0;
        }
    }
}

// ------------------------------------------------------------------ host side
static std::atomic<int> g_fused_timing{0};
void set_fused_timing(int v) { g_fused_timing.store(v ? 1 : 0, std::memory_order_relaxed); }

struct FusedWork {
    dev_buf<double> acc;       // [m]: F so far; the batched form: [G][m], a row per need of the group in flight
    dev_buf<double> par;       // the call's parameters, one upload: [j] weights, then [j] int32 flags (1 for a served vector); the
                               // batched form: [nv] weights, [b + 1] int64 offsets, [b] int64 first, [b] int64 last, [nv] int32 flags
    pin_buf<double> hpar;      // pinned staging of the same
    dev_events<2> ev;          // made by the first call under "fused_timing"
    int64_t j = 0;             // vectors of the call in flight
    const int32_t* hflags() const { return (const int32_t*)((const double*)hpar + j); }
};

void fused_work_free(FusedWork* f) { delete f; }

as_status fused_begin(SubsetWork* w, int64_t m, int64_t j, const double* weights, const int32_t* status, int mode, FusedCall* c) {
    if (!w->fused) {
        w->fused = new (std::nothrow) FusedWork();
        if (!w->fused) {
            set_err("fused: out of host memory");
            return AS_ENOMEM;
        }
    }
    FusedWork* f = w->fused;
    c->w = w;
    c->m = m;
    c->mode = mode;
    c->fresh = true;
    c->timing = g_fused_timing.load(std::memory_order_relaxed) != 0;
    c->timed = false;
    c->launches = c->folded = 0;
    c->us = 0.0;
    if (c->timing && !f->ev.e[1]) AS_HIP(f->ev.create());
    AS_TRY(reserve_or_err(f->acc, std::max<int64_t>(m, 1), "fused accumulator"));
    const int64_t words = j + (j + 1) / 2;   // doubles: the weights, then the flags two to a double
    AS_TRY(reserve_or_err(f->par, words, "fused weights and flags"));
    AS_TRY(reserve_or_err(f->hpar, words, "fused pinned weights and flags"));
    f->j = j;
    int32_t* hflags = (int32_t*)((double*)f->hpar + j);
    for (int64_t t = 0; t < j; ++t) {
        f->hpar[t] = weights[t];
        hflags[t] = status[t] == AS_EZEROLAMBDA ? 0 : 1;
    }
    AS_HIP(hipMemcpyAsync(f->par, f->hpar, sizeof(double) * (size_t)j + sizeof(int32_t) * (size_t)j, hipMemcpyHostToDevice, w->stream));
    return AS_OK;
}

// the time of the launch before this one: the stream has been waited for since (one pair of events serves every chunk)
template <typename Call>
static as_status fused_collect_time(Call* c) {
    if (!c->timed) return AS_OK;
    float ms = 0.0f;
    AS_HIP(hipEventElapsedTime(&ms, c->w->fused->ev.e[0], c->w->fused->ev.e[1]));
    c->us += (double)ms * 1e3;
    c->timed = false;
    return AS_OK;
}

as_status fused_chunk(FusedCall* c, int64_t i0, int64_t nb, const double* scores, int64_t ld) {
    SubsetWork* w = c->w;
    FusedWork* f = w->fused;
    int64_t served = 0;
    for (int64_t t = 0; t < nb; ++t) served += f->hflags()[i0 + t];
    if (served == 0 || c->m <= 0) return AS_OK;
    AS_TRY(fused_collect_time(c));
    const int64_t units = (c->m + 1) / 2;
    const unsigned grid = (unsigned)filtered_grid(std::max<int64_t>(1, std::min<int64_t>((units + FA_THREADS - 1) / FA_THREADS, (int64_t)w->cus * FA_BLOCKS_PER_CU)));
    const double* wts = f->par + i0;
    const int32_t* flags = (const int32_t*)((const double*)f->par + f->j) + i0;
    double* acc = f->acc;
    if (c->timing) AS_HIP(hipEventRecord(f->ev.e[0], w->stream));
    if (c->mode == 0)
        hipLaunchKernelGGL(fused_accumulate_kernel<0>, dim3(grid), dim3(FA_THREADS), 0, w->stream, scores, ld, c->m, (int)nb, wts, flags, acc,
                           c->fresh ? 1 : 0);
    else
        hipLaunchKernelGGL(fused_accumulate_kernel<1>, dim3(grid), dim3(FA_THREADS), 0, w->stream, scores, ld, c->m, (int)nb, wts, flags, acc,
                           c->fresh ? 1 : 0);
    AS_HIP(hipGetLastError());
    if (c->timing) {
        AS_HIP(hipEventRecord(f->ev.e[1], w->stream));
        c->timed = true;
    }
    c->fresh = false;
    c->launches += 1;
    c->folded += served * c->m;
    return AS_OK;
}

as_status fused_end(FusedCall* c) { return fused_collect_time(c); }

const double* fused_acc(const SubsetWork* w) { return w->fused ? (const double*)w->fused->acc : nullptr; }

// ------------------------------------------------------------------ the batched form (S15, section 5.18)
static std::atomic<int> g_fused_batch_timing{0};
static std::atomic<int> g_fused_batch_mib{256};
void set_fused_batch_timing(int v) { g_fused_batch_timing.store(v ? 1 : 0, std::memory_order_relaxed); }
void set_fused_batch_mib(int v) { g_fused_batch_mib.store(v != 0 ? v : 256, std::memory_order_relaxed); }

as_status fused_batch_begin(SubsetWork* w, int64_t m, int64_t b, const int64_t* offs, const double* weights, const int32_t* status, int mode,
                            FusedBatchCall* c) {
    if (!w->fused) {
        w->fused = new (std::nothrow) FusedWork();
        if (!w->fused) {
            set_err("fused: out of host memory");
            return AS_ENOMEM;
        }
    }
    FusedWork* f = w->fused;
    const int64_t nv = offs[b];
    c->w = w;
    c->m = m;
    c->b = b;
    c->nv = nv;
    c->mode = mode;
    c->g0 = c->gn = 0;
    c->timing = g_fused_batch_timing.load(std::memory_order_relaxed) != 0;
    c->timed = false;
    c->launches = c->folded = c->groups = 0;
    c->us = 0.0;
    // needs per group: the accumulator rows that fit the budget (v > 0: MiB; v < 0: -v KiB, for tests at small shapes)
    const int v = g_fused_batch_mib.load(std::memory_order_relaxed);
    const int64_t budget = v > 0 ? (int64_t)v << 20 : (int64_t)(-(int64_t)v) << 10;
    const int64_t row = std::max<int64_t>(m, 1) * (int64_t)sizeof(double);
    c->gmax = std::min<int64_t>(std::min<int64_t>(std::max<int64_t>(budget / row, 1), SB_QC_MAX), b);
    if (c->timing && !f->ev.e[1]) AS_HIP(f->ev.create());
    AS_TRY(reserve_or_err(f->acc, std::max<int64_t>(c->gmax * m, 1), "fused accumulators"));
    const int64_t words = BatchPar::words(nv, b);
    AS_TRY(reserve_or_err(f->par, words, "fused weights, segments and flags"));
    AS_TRY(reserve_or_err(f->hpar, words, "fused pinned weights, segments and flags"));
    f->j = 0;
    (void)BatchPar(f->hpar, nv, b).fill(b, offs, weights, status);
    AS_HIP(hipMemcpyAsync(f->par, f->hpar, BatchPar::bytes(nv, b), hipMemcpyHostToDevice, w->stream));
    return AS_OK;
}

void fused_batch_group(FusedBatchCall* c, int64_t g0, int64_t gn) {
    c->g0 = g0;
    c->gn = gn;
    c->groups += 1;
}

as_status fused_batch_chunk(FusedBatchCall* c, int64_t i0, int64_t nb, const double* scores, int64_t ld) {
    SubsetWork* w = c->w;
    FusedWork* f = w->fused;
    const BatchPar h(f->hpar, c->nv, c->b), dv(f->par, c->nv, c->b);
    const int64_t r0 = h.offs[c->g0] + i0;   // the chunk's rows as flattened rows of the call
    if (nb <= 0 || c->m <= 0 || r0 + nb > h.offs[c->g0 + c->gn]) return AS_OK;   // (rows of the group in flight only)
    int64_t served = 0;
    for (int64_t t = 0; t < nb; ++t) served += h.flags[r0 + t];
    if (served == 0) return AS_OK;
    // the needs the chunk touches: the one that holds row r0 .. the one that holds row r0 + nb - 1
    const int64_t need0 = (std::upper_bound(h.offs, h.offs + c->b + 1, r0) - h.offs) - 1;
    const int64_t need1 = (std::upper_bound(h.offs, h.offs + c->b + 1, r0 + nb - 1) - h.offs) - 1;
    AS_TRY(fused_collect_time(c));
    const int64_t units = (c->m + 1) / 2;
    const dim3 grid((unsigned)filtered_grid(std::max<int64_t>(1, std::min<int64_t>((units + FA_THREADS - 1) / FA_THREADS, (int64_t)w->cus * FA_BLOCKS_PER_CU))),
                    (unsigned)(need1 - need0 + 1));
    double* acc = f->acc;
    if (c->timing) AS_HIP(hipEventRecord(f->ev.e[0], w->stream));
    if (c->mode == 0)
        hipLaunchKernelGGL(fused_accumulate_batch_kernel<0>, grid, dim3(FA_THREADS), 0, w->stream, scores, ld, c->m, r0, (int)nb, need0, c->g0,
                           (const int64_t*)dv.offs, (const int64_t*)dv.first, (const int64_t*)dv.last, (const double*)dv.wts,
                           (const int32_t*)dv.flags, acc);
    else
        hipLaunchKernelGGL(fused_accumulate_batch_kernel<1>, grid, dim3(FA_THREADS), 0, w->stream, scores, ld, c->m, r0, (int)nb, need0, c->g0,
                           (const int64_t*)dv.offs, (const int64_t*)dv.first, (const int64_t*)dv.last, (const double*)dv.wts,
                           (const int32_t*)dv.flags, acc);
    AS_HIP(hipGetLastError());
    if (c->timing) {
        AS_HIP(hipEventRecord(f->ev.e[1], w->stream));
        c->timed = true;
    }
    c->launches += 1;
    c->folded += served * c->m;
    return AS_OK;
}

as_status fused_batch_end(FusedBatchCall* c) { return fused_collect_time(c); }

}  // namespace as
