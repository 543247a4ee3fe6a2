// Late-interaction search: ONE answer to J query vectors over GROUPS of items -- F(g) = the sum over
// the vectors j of w_j x the largest score of group g's members under vector j (the MaxSim rule of ColBERT-style retrievers).  The
// scores come from the batched filtered forms' score kernel (as_subset.hip), unchanged, a chunk of vectors at a time; pass A of
// round 0 of grouped search's pick kernel (as_grouped.hip, group_max_launch), unchanged, turns each row of the chunk into one
// sel_ord key per group (0: no member); this file's kernel decodes the keys and folds the chunk's [nb][G] cells into one
// accumulator [G] that stays on the device and carries over the chunks (maxsim_fold_kernel), by S13's step (as_fused_step.hpp).  The
// filtered forms' exact selection over the accumulator, position == dense group number, names the best groups.
// Entry points: as_api.hip (as_search_maxsim, as_score_maxsim, as_maxsim_counters, as_maxsim_kernel_us).
// The batched form (S17, section 5.20): B needs of J_b vectors each in one call.  The vectors of all needs are ONE flattened list of
// rows for the score kernel and for pass A; maxsim_fold_batch_kernel folds each chunk's cells segment by segment into one
// accumulator row per need ([Gn][G], Gn needs at a time); the search form selects over the rows at once, the score form picks the
// listed groups on the device (maxsim_pick_kernel).  Entry points: as_search_maxsim_batch, as_score_maxsim_batch,
// as_maxsim_batch_counters, as_maxsim_batch_kernel_us.
#include <algorithm>
#include <atomic>
#include <new>
#include <vector>

#include "as_common.hpp"
#include "as_fused_step.hpp"   // fused_step; from here on nothing is contracted into an FMA

namespace as {

// a pair of cells of one row: rows start on an 8-byte boundary only (G may be odd), so the type promises no more than that; the
// load is still one 16-byte instruction
typedef unsigned long long u64x2_a8 __attribute__((ext_vector_type(2), aligned(8)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int MS_THREADS = 256;
constexpr int MS_ROWS = 8;             // rows whose loads are in flight together
constexpr int MS_BLOCKS_PER_CU = 8;    // the grid: that many blocks per CU at most, the rest is the grid-stride loop

// the double a sel_ord key stands for: key 0 (no member) is a NaN; -0.0 went in as +0.0 and comes out as +0.0
__device__ __forceinline__ double maxsim_decode(unsigned long long key) {
    if (key == 0ull) return __longlong_as_double(0x7ff8000000000000LL);
    const unsigned long long b = (key & 0x8000000000000000ull) ? (key & 0x7fffffffffffffffull) : ~key;
    return __longlong_as_double((long long)b);
}

// acc[g] <- the S13 sum of rows 0 .. nb - 1 of the cells ([nb][G] sel_ord keys, the group maxima of pass A) at group g < G onto
// acc[g], rows ascending; a row whose flag is 0 is skipped (wave-uniform: the flags are the same for every lane).  fresh: the
// accumulator holds nothing yet -- the first served row of the chunk initialises it (no memset, no 0 + t).  A thread owns a pair
// of neighbouring groups (16-byte loads and stores; the accumulator is 16-byte aligned) for all rows, so no two threads meet in a
// group and the stores are plain; an odd G leaves one single group to the thread behind the last pair.  No LDS, no atomics, no
// barrier.
__global__ __launch_bounds__(MS_THREADS) void maxsim_fold_kernel(const unsigned long long* __restrict__ cells, int64_t G, int nb,
                                                                 const double* __restrict__ wts, const int32_t* __restrict__ flags,
                                                                 double* __restrict__ acc, int fresh) {
    const int64_t pairs = G >> 1, units = pairs + (G & 1);
    for (int64_t u = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; u < units; u += (int64_t)gridDim.x * MS_THREADS) {
        const bool pair = u < pairs;
        const int64_t g = 2 * u;   // (the single group of an odd G: g == G - 1)
        bool have = fresh == 0;
        double f0 = 0.0, f1 = 0.0;
        if (have) {
            if (pair) {
                const f64x2 a = *(const f64x2*)(acc + g);
                f0 = a[0];
                f1 = a[1];
            } else {
                f0 = acc[g];
            }
        }
        for (int j0 = 0; j0 < nb; j0 += MS_ROWS) {
            unsigned long long k0[MS_ROWS], k1[MS_ROWS];
#pragma unroll
            for (int r = 0; r < MS_ROWS; ++r) {
                k0[r] = 0ull;
                k1[r] = 0ull;
                if (j0 + r < nb) {
                    const unsigned long long* p = cells + (int64_t)(j0 + r) * G + g;
                    if (pair) {
                        const u64x2_a8 x = *(const u64x2_a8*)p;
                        k0[r] = x[0];
                        k1[r] = x[1];
                    } else {
                        k0[r] = *p;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < MS_ROWS; ++r) {
                if (j0 + r < nb && flags[j0 + r]) {
                    const double wj = wts[j0 + r];
                    f0 = fused_step<0>(f0, wj, maxsim_decode(k0[r]), have);
                    f1 = fused_step<0>(f1, wj, maxsim_decode(k1[r]), have);
                    have = true;
                }
            }
        }
        if (!have) continue;   // (no served row so far: the host does not launch such a chunk)
        if (pair) {
            f64x2 o;
            o[0] = f0;
            o[1] = f1;
            *(f64x2*)(acc + g) = o;
        } else {
            acc[g] = f0;
        }
    }
}

// The segmented fold of the batched form (S17, section 5.20): fused_accumulate_batch_kernel<0> (as_fused.hip) with the decode
// above in front.  The chunk's cells ([nb][G] sel_ord keys) hold the flattened rows r0 .. r0 + nb - 1 of the call; need
// y = need0 + blockIdx.y owns rows offs[y] .. offs[y + 1] - 1 of them, cut by the chunk's edges, and the accumulator row
// acc + (y - gneed0) * G.  first[y] / last[y]: the flattened index of the need's first / last served row (-1: none) -- the need's
// accumulator holds something iff its first served row lies before the rows taken here, so no launch has to be told; a need
// without a served row at or before / at or behind this chunk leaves at once (block-uniform: y is).  Inside a need the kernel is
// maxsim_fold_kernel: a thread owns a pair of neighbouring groups for all the need's rows of the chunk, MS_ROWS loads in flight,
// rows ascending, plain 16-byte stores.  An accumulator row starts on an 8-byte boundary only (G may be odd): f64x2_a8.
typedef double f64x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

__global__ __launch_bounds__(MS_THREADS) void maxsim_fold_batch_kernel(const unsigned long long* __restrict__ cells, int64_t G, int64_t r0, int nb,
                                                                       int64_t need0, int64_t gneed0, const int64_t* __restrict__ offs,
                                                                       const int64_t* __restrict__ first, const int64_t* __restrict__ last,
                                                                       const double* __restrict__ wts, const int32_t* __restrict__ flags,
                                                                       double* __restrict__ acc) {
    const int64_t need = need0 + blockIdx.y;
    const int64_t o0 = offs[need], o1 = offs[need + 1];
    const int64_t lo = o0 > r0 ? o0 : r0, hi = o1 < r0 + nb ? o1 : r0 + nb;
    const int64_t fs = first[need];
    if (fs < 0 || fs >= hi || last[need] < lo) return;
    const bool carried = fs < lo;
    const int n = (int)(hi - lo);
    const unsigned long long* __restrict__ rows = cells + (lo - r0) * G;
    const double* __restrict__ w = wts + lo;
    const int32_t* __restrict__ fl = flags + lo;
    double* __restrict__ a = acc + (need - gneed0) * G;
    const int64_t pairs = G >> 1, units = pairs + (G & 1);
    for (int64_t u = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; u < units; u += (int64_t)gridDim.x * MS_THREADS) {
        const bool pair = u < pairs;
        const int64_t g = 2 * u;   // (the single group of an odd G: g == G - 1)
        bool have = carried;
        double f0 = 0.0, f1 = 0.0;
        if (have) {
            if (pair) {
                const f64x2_a8 x = *(const f64x2_a8*)(a + g);
                f0 = x[0];
                f1 = x[1];
            } else {
                f0 = a[g];
            }
        }
        bool touched = false;
        for (int j0 = 0; j0 < n; j0 += MS_ROWS) {
            unsigned long long k0[MS_ROWS], k1[MS_ROWS];
#pragma unroll
            for (int r = 0; r < MS_ROWS; ++r) {
                k0[r] = 0ull;
                k1[r] = 0ull;
                if (j0 + r < n) {
                    const unsigned long long* p = rows + (int64_t)(j0 + r) * G + g;
                    if (pair) {
                        const u64x2_a8 x = *(const u64x2_a8*)p;
                        k0[r] = x[0];
                        k1[r] = x[1];
                    } else {
                        k0[r] = *p;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < MS_ROWS; ++r) {
                if (j0 + r < n && fl[j0 + r]) {
                    const double wj = w[j0 + r];
                    f0 = fused_step<0>(f0, wj, maxsim_decode(k0[r]), have);
                    f1 = fused_step<0>(f1, wj, maxsim_decode(k1[r]), have);
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
            *(f64x2_a8*)(a + g) = o;
        } else {
            a[g] = f0;
        }
    }
}

// The score form of the batched call: out[y][l] <- acc[y][gnum[l]] for the needs y < gridDim.y of the group in flight and the
// nl listed groups (gnum: their dense group numbers, checked on the host), so that only the listed F cross to the host.
__global__ __launch_bounds__(MS_THREADS) void maxsim_pick_kernel(const double* __restrict__ acc, int64_t G, const int32_t* __restrict__ gnum,
                                                                 int64_t nl, double* __restrict__ out) {
    const double* __restrict__ a = acc + (int64_t)blockIdx.y * G;
    double* __restrict__ o = out + (int64_t)blockIdx.y * nl;
    for (int64_t l = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; l < nl; l += (int64_t)gridDim.x * MS_THREADS) o[l] = a[gnum[l]];
}

// ------------------------------------------------------------------ host side
static std::atomic<int> g_maxsim_timing{0};
void set_maxsim_timing(int v) { g_maxsim_timing.store(v ? 1 : 0, std::memory_order_relaxed); }

struct MaxsimWork {
    dev_buf<unsigned long long> cells;   // [nb][G]: the chunk's group maxima as sel_ord keys, zeroed inside the call
    dev_buf<double> acc;                 // [G]: F so far; the batched form: [Gn][G], a row per need of the group in flight
    dev_buf<double> par;                 // the call's parameters, one upload: [j] weights, then [j] int32 flags (1 for a served vector);
                                         // the batched form: BatchPar's layout
    pin_buf<double> hpar;                // pinned staging of the same
    dev_buf<int32_t> gnum;               // the batched score form: [nl] dense group numbers of the listed labels
    dev_buf<double> picked;              // ... and [Gn][nl]: the listed F of the group in flight
    dev_buf<int32_t> ident;              // [ident_n] position -> group number of the selection: the identity
    int64_t ident_n = 0;
    dev_buf<unsigned long long> natom;   // [1]
    pin_buf<unsigned long long> hnatom;  // [1]
    dev_events<3> ev;                    // made by the first call under "maxsim_timing": before pass A, between, behind the fold
    int64_t j = 0;                       // vectors of the call in flight
    const int32_t* hflags() const { return (const int32_t*)((const double*)hpar + j); }
};

void maxsim_work_free(MaxsimWork* x) { delete x; }

as_status maxsim_begin(SubsetWork* w, const as_groups* gs, int64_t m, int64_t j, const double* weights, const int32_t* status, MaxsimCall* c) {
    if (!w->maxsim) {
        w->maxsim = new (std::nothrow) MaxsimWork();
        if (!w->maxsim) {
            set_err("maxsim: out of host memory");
            return AS_ENOMEM;
        }
    }
    MaxsimWork* x = w->maxsim;
    c->w = w;
    c->g = gs;
    c->m = m;
    c->fresh = true;
    c->timing = g_maxsim_timing.load(std::memory_order_relaxed) != 0;
    c->timed = false;
    c->served = c->passa = c->atoms = c->folds = 0;
    c->us[0] = c->us[1] = 0.0;
    if (c->timing && !x->ev.e[2]) AS_HIP(x->ev.create());
    AS_TRY(reserve_or_err(x->acc, std::max<int64_t>(gs->count, 1), "maxsim accumulator"));
    AS_TRY(reserve_or_err(x->natom, 1, "maxsim counter"));
    AS_TRY(reserve_or_err(x->hnatom, 1, "maxsim pinned counter"));
    const int64_t words = j + (j + 1) / 2;   // doubles: the weights, then the flags two to a double
    AS_TRY(reserve_or_err(x->par, words, "maxsim weights and flags"));
    AS_TRY(reserve_or_err(x->hpar, words, "maxsim pinned weights and flags"));
    x->j = j;
    int32_t* hflags = (int32_t*)((double*)x->hpar + j);
    for (int64_t t = 0; t < j; ++t) {
        x->hpar[t] = weights[t];
        hflags[t] = status[t] == AS_EZEROLAMBDA ? 0 : 1;
        c->served += hflags[t];
    }
    x->hnatom[0] = 0ull;
    AS_HIP(hipMemcpyAsync(x->par, x->hpar, sizeof(double) * (size_t)j + sizeof(int32_t) * (size_t)j, hipMemcpyHostToDevice, w->stream));
    AS_HIP(hipMemsetAsync(x->natom, 0, sizeof(unsigned long long), w->stream));
    return AS_OK;
}

// the times of the launches before this point: the stream has been waited for since (one set of events serves every chunk)
template <typename Call>
static as_status maxsim_collect_time(Call* c) {
    if (!c->timed) return AS_OK;
    const MaxsimWork* x = c->w->maxsim;
    for (int t = 0; t < 2; ++t) {
        float ms = 0.0f;
        AS_HIP(hipEventElapsedTime(&ms, x->ev.e[t], x->ev.e[t + 1]));
        c->us[t] += (double)ms * 1e3;
    }
    c->timed = false;
    return AS_OK;
}

as_status maxsim_chunk(MaxsimCall* c, int64_t i0, int64_t nb, const double* scores, int64_t ld) {
    SubsetWork* w = c->w;
    MaxsimWork* x = w->maxsim;
    const int64_t G = c->g->count;
    const int32_t* hf = x->hflags() + i0;
    int64_t served = 0;
    for (int64_t t = 0; t < nb; ++t) served += hf[t];
    if (served == 0 || c->m <= 0 || G <= 0) return AS_OK;
    AS_TRY(maxsim_collect_time(c));
    AS_TRY(reserve_or_err(x->cells, nb * G, "maxsim cells"));   // (the first chunk of a call is its largest)
    unsigned long long* cells = x->cells;
    unsigned long long* natom = x->natom;
    if (c->timing) AS_HIP(hipEventRecord(x->ev.e[0], w->stream));
    AS_HIP(hipMemsetAsync(cells, 0, sizeof(unsigned long long) * (size_t)(nb * G), w->stream));
    for (int64_t t = 0; t < nb;) {   // pass A over every maximal run of served rows: an unserved row's scores are no answer
        if (!hf[t]) {
            ++t;
            continue;
        }
        int64_t u = t;
        while (u < nb && hf[u]) ++u;
        AS_TRY(group_max_launch(w, c->g, scores + t * ld, ld, c->m, u - t, cells + t * G, natom));
        c->passa += 1;
        t = u;
    }
    if (c->timing) AS_HIP(hipEventRecord(x->ev.e[1], w->stream));
    const int64_t units = (G + 1) / 2;
    const unsigned grid = (unsigned)filtered_grid(std::max<int64_t>(1, std::min<int64_t>((units + MS_THREADS - 1) / MS_THREADS, (int64_t)w->cus * MS_BLOCKS_PER_CU)));
    const double* wts = x->par + i0;
    const int32_t* flags = (const int32_t*)((const double*)x->par + x->j) + i0;
    double* acc = x->acc;
    hipLaunchKernelGGL(maxsim_fold_kernel, dim3(grid), dim3(MS_THREADS), 0, w->stream, (const unsigned long long*)cells, G, (int)nb, wts, flags, acc,
                       c->fresh ? 1 : 0);
    AS_HIP(hipGetLastError());
    if (c->timing) {
        AS_HIP(hipEventRecord(x->ev.e[2], w->stream));
        c->timed = true;
    }
    c->fresh = false;
    c->folds += 1;
    return AS_OK;
}

// the identity table of the selection for G positions: filled when it grows, kept
static as_status maxsim_identity(SubsetWork* w, int64_t G) {
    MaxsimWork* x = w->maxsim;
    if (x->ident_n >= G) return AS_OK;
    x->ident_n = 0;
    AS_TRY(reserve_or_err(x->ident, G, "maxsim group numbers"));
    std::vector<int32_t> h;
    try {
        h.resize((size_t)G);
    } catch (const std::bad_alloc&) {
        set_err("maxsim: out of host memory for %lld group numbers", (long long)G);
        return AS_ENOMEM;
    }
    for (int64_t g = 0; g < G; ++g) h[(size_t)g] = (int32_t)g;
    AS_HIP(hipMemcpyAsync(x->ident, h.data(), sizeof(int32_t) * (size_t)G, hipMemcpyHostToDevice, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));   // (h goes away)
    x->ident_n = G;
    return AS_OK;
}

as_status maxsim_select(MaxsimCall* c, int64_t k, int64_t* out_group, double* out_score, int64_t* out_len) {
    SubsetWork* w = c->w;
    MaxsimWork* x = w->maxsim;
    *out_len = 0;
    if (c->fresh) {   // (nothing was folded: no answer)
        AS_HIP(hipStreamSynchronize(w->stream));
        return AS_OK;
    }
    AS_TRY(maxsim_identity(w, c->g->count));
    AS_HIP(hipMemcpyAsync(x->hnatom, x->natom, sizeof(unsigned long long), hipMemcpyDeviceToHost, w->stream));
    AS_TRY(subset_select_from_table(w, x->acc, x->ident, c->g->count, k, out_group, out_score, out_len));   // waits
    c->atoms = (int64_t)x->hnatom[0];
    return maxsim_collect_time(c);
}

as_status maxsim_scores(MaxsimCall* c, double* out) {
    SubsetWork* w = c->w;
    MaxsimWork* x = w->maxsim;
    if (!c->fresh) {
        AS_HIP(hipMemcpyAsync(out, x->acc, sizeof(double) * (size_t)c->g->count, hipMemcpyDeviceToHost, w->stream));
        AS_HIP(hipMemcpyAsync(x->hnatom, x->natom, sizeof(unsigned long long), hipMemcpyDeviceToHost, w->stream));
    }
    AS_HIP(hipStreamSynchronize(w->stream));
    c->atoms = (int64_t)x->hnatom[0];
    return maxsim_collect_time(c);
}

// ------------------------------------------------------------------ the batched form (S17, section 5.20)
static std::atomic<int> g_maxsim_batch_timing{0};
static std::atomic<int> g_maxsim_batch_mib{256};
void set_maxsim_batch_timing(int v) { g_maxsim_batch_timing.store(v ? 1 : 0, std::memory_order_relaxed); }
void set_maxsim_batch_mib(int v) { g_maxsim_batch_mib.store(v != 0 ? v : 256, std::memory_order_relaxed); }

as_status maxsim_batch_begin(SubsetWork* w, const as_groups* gs, int64_t m, int64_t b, const int64_t* offs, const double* weights,
                             const int32_t* status, MaxsimBatchCall* c) {
    if (!w->maxsim) {
        w->maxsim = new (std::nothrow) MaxsimWork();
        if (!w->maxsim) {
            set_err("maxsim: out of host memory");
            return AS_ENOMEM;
        }
    }
    MaxsimWork* x = w->maxsim;
    const int64_t nv = offs[b], G = gs->count;
    c->w = w;
    c->g = gs;
    c->m = m;
    c->b = b;
    c->nv = nv;
    c->g0 = c->gn = 0;
    c->timing = g_maxsim_batch_timing.load(std::memory_order_relaxed) != 0;
    c->timed = false;
    c->served = c->passa = c->atoms = c->folds = c->groups = 0;
    c->us[0] = c->us[1] = 0.0;
    // needs per group: the accumulator rows that fit the budget (v > 0: MiB; v < 0: -v KiB, for tests at small shapes)
    const int v = g_maxsim_batch_mib.load(std::memory_order_relaxed);
    const int64_t budget = v > 0 ? (int64_t)v << 20 : (int64_t)(-(int64_t)v) << 10;
    const int64_t row = std::max<int64_t>(G, 1) * (int64_t)sizeof(double);
    c->gmax = std::min<int64_t>(std::min<int64_t>(std::max<int64_t>(budget / row, 1), SB_QC_MAX), b);
    if (c->timing && !x->ev.e[2]) AS_HIP(x->ev.create());
    AS_TRY(reserve_or_err(x->acc, std::max<int64_t>(c->gmax * G, 1), "maxsim accumulators"));
    AS_TRY(reserve_or_err(x->natom, 1, "maxsim counter"));
    AS_TRY(reserve_or_err(x->hnatom, 1, "maxsim pinned counter"));
    const int64_t words = BatchPar::words(nv, b);
    AS_TRY(reserve_or_err(x->par, words, "maxsim weights, segments and flags"));
    AS_TRY(reserve_or_err(x->hpar, words, "maxsim pinned weights, segments and flags"));
    x->j = 0;
    c->served = BatchPar(x->hpar, nv, b).fill(b, offs, weights, status);
    x->hnatom[0] = 0ull;
    AS_HIP(hipMemcpyAsync(x->par, x->hpar, BatchPar::bytes(nv, b), hipMemcpyHostToDevice, w->stream));
    AS_HIP(hipMemsetAsync(x->natom, 0, sizeof(unsigned long long), w->stream));
    return AS_OK;
}

as_status maxsim_batch_labels(MaxsimBatchCall* c, const int32_t* gnum_host, int64_t nl) {
    SubsetWork* w = c->w;
    MaxsimWork* x = w->maxsim;
    c->nl = nl;
    AS_TRY(reserve_or_err(x->gnum, std::max<int64_t>(nl, 1), "maxsim listed groups"));
    AS_TRY(reserve_or_err(x->picked, std::max<int64_t>(c->gmax * nl, 1), "maxsim listed scores"));
    AS_HIP(hipMemcpyAsync(x->gnum, gnum_host, sizeof(int32_t) * (size_t)nl, hipMemcpyHostToDevice, w->stream));
    return AS_OK;
}

void maxsim_batch_group(MaxsimBatchCall* c, int64_t g0, int64_t gn) {
    c->g0 = g0;
    c->gn = gn;
    c->groups += 1;
}

as_status maxsim_batch_chunk(MaxsimBatchCall* c, int64_t i0, int64_t nb, const double* scores, int64_t ld) {
    SubsetWork* w = c->w;
    MaxsimWork* x = w->maxsim;
    const int64_t G = c->g->count;
    const BatchPar h(x->hpar, c->nv, c->b), dv(x->par, c->nv, c->b);
    const int64_t r0 = h.offs[c->g0] + i0;   // the chunk's rows as flattened rows of the call
    if (nb <= 0 || c->m <= 0 || G <= 0 || r0 + nb > h.offs[c->g0 + c->gn]) return AS_OK;   // (rows of the group in flight only)
    const int32_t* hf = h.flags + r0;
    int64_t served = 0;
    for (int64_t t = 0; t < nb; ++t) served += hf[t];
    if (served == 0) return AS_OK;
    // the needs the chunk touches: the one that holds row r0 .. the one that holds row r0 + nb - 1
    const int64_t need0 = (std::upper_bound(h.offs, h.offs + c->b + 1, r0) - h.offs) - 1;
    const int64_t need1 = (std::upper_bound(h.offs, h.offs + c->b + 1, r0 + nb - 1) - h.offs) - 1;
    AS_TRY(maxsim_collect_time(c));
    AS_TRY(reserve_or_err(x->cells, nb * G, "maxsim cells"));   // (the first chunk of a group is its largest)
    unsigned long long* cells = x->cells;
    unsigned long long* natom = x->natom;
    if (c->timing) AS_HIP(hipEventRecord(x->ev.e[0], w->stream));
    AS_HIP(hipMemsetAsync(cells, 0, sizeof(unsigned long long) * (size_t)(nb * G), w->stream));
    for (int64_t t = 0; t < nb;) {   // pass A over every maximal run of served rows, whatever need they belong to
        if (!hf[t]) {
            ++t;
            continue;
        }
        int64_t u = t;
        while (u < nb && hf[u]) ++u;
        AS_TRY(group_max_launch(w, c->g, scores + t * ld, ld, c->m, u - t, cells + t * G, natom));
        c->passa += 1;
        t = u;
    }
    if (c->timing) AS_HIP(hipEventRecord(x->ev.e[1], w->stream));
    const int64_t units = (G + 1) / 2;
    const dim3 grid((unsigned)filtered_grid(std::max<int64_t>(1, std::min<int64_t>((units + MS_THREADS - 1) / MS_THREADS, (int64_t)w->cus * MS_BLOCKS_PER_CU))),
                    (unsigned)(need1 - need0 + 1));
    double* acc = x->acc;
    hipLaunchKernelGGL(maxsim_fold_batch_kernel, grid, dim3(MS_THREADS), 0, w->stream, (const unsigned long long*)cells, G, r0, (int)nb, need0, c->g0,
                       (const int64_t*)dv.offs, (const int64_t*)dv.first, (const int64_t*)dv.last, (const double*)dv.wts, (const int32_t*)dv.flags,
                       acc);
    AS_HIP(hipGetLastError());
    if (c->timing) {
        AS_HIP(hipEventRecord(x->ev.e[2], w->stream));
        c->timed = true;
    }
    c->folds += 1;
    return AS_OK;
}

as_status maxsim_batch_select(MaxsimBatchCall* c, int64_t k) {
    SubsetWork* w = c->w;
    MaxsimWork* x = w->maxsim;
    const int64_t G = c->g->count;
    AS_TRY(maxsim_identity(w, G));
    return subset_select_rows_from(w, x->acc, x->ident, G, G, k, c->gn);   // waits
}

as_status maxsim_batch_pick(MaxsimBatchCall* c, double* out) {
    SubsetWork* w = c->w;
    MaxsimWork* x = w->maxsim;
    const int64_t nl = c->nl;
    if (nl <= 0 || c->gn <= 0) return AS_OK;
    const dim3 grid((unsigned)filtered_grid(std::max<int64_t>(1, std::min<int64_t>((nl + MS_THREADS - 1) / MS_THREADS, (int64_t)w->cus * MS_BLOCKS_PER_CU))),
                    (unsigned)c->gn);
    double* picked = x->picked;
    hipLaunchKernelGGL(maxsim_pick_kernel, grid, dim3(MS_THREADS), 0, w->stream, (const double*)x->acc, c->g->count, (const int32_t*)x->gnum, nl,
                       picked);
    AS_HIP(hipGetLastError());
    AS_HIP(hipMemcpyAsync(out, picked, sizeof(double) * (size_t)(c->gn * nl), hipMemcpyDeviceToHost, w->stream));
    return AS_OK;
}

as_status maxsim_batch_end(MaxsimBatchCall* c) {
    SubsetWork* w = c->w;
    MaxsimWork* x = w->maxsim;
    AS_HIP(hipMemcpyAsync(x->hnatom, x->natom, sizeof(unsigned long long), hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    c->atoms = (int64_t)x->hnatom[0];
    return maxsim_collect_time(c);
}

}  // namespace as
