// Filtered search: the exact S11 scores of a list of items gathered by id (subset_score_kernel) and the
// exact top-k of them by (score descending, position ascending) -- a radix select over an order-preserving 96-bit key (the
// score's bits, then the inverted position: no two keys are equal), then a one-block sort of the k selected entries.
// Entry points: as_api.hip (as_search_subset, as_score_items).
#include <algorithm>
#include <new>

#include "as_common.hpp"

namespace as {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SUB_ROWS = 4;        // rows in flight per wave: every load of the four is issued before the first FMA
constexpr int SUB_Q_LDS = 4096;    // the query sits in LDS up to this many doubles (32 KiB a block); longer ones are read from global memory
constexpr int SUB_BLOCKS_PER_CU = 4;   // 4 blocks of 4 waves: 16 waves per CU

struct SubsetArgs {
    const int32_t* ids;
    int64_t m;
    const float* x32;
    const double* x64;
    const double* n64;
    const double* lam64;
    const double* q64;
    double* scores;
    int64_t d, dp;
    double nq, lq, tau;
};

// One wave per row, SUB_ROWS rows at a time, grid-stride over the id list; the ids are wave-uniform.  F64: the rows are the fp64
// items ([n][d], rows 8-byte aligned: one double per lane and load); else the fp32 items ([np][dp], zero padded, dp a multiple of
// 32: 16 bytes per lane and load), widened before the product.  QLDS: the query is staged in LDS once per block.
template <bool F64, bool QLDS>
__global__ __launch_bounds__(256) void subset_score_kernel(SubsetArgs a) {
    extern __shared__ double qs[];
    if (QLDS) {
        for (int64_t c = threadIdx.x; c < a.dp; c += blockDim.x) qs[c] = a.q64[c];
        __syncthreads();
    }
    const int lane = lane_id();
    // (the wave's number as a scalar: the id loads below are scalar loads then)
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t step = (int64_t)gridDim.x * (blockDim.x >> 6) * SUB_ROWS;
    int32_t next[SUB_ROWS];   // the ids of the next group: loaded one trip ahead, no id load in front of a trip's row loads
#pragma unroll
    for (int r = 0; r < SUB_ROWS; ++r) next[r] = a.ids[min(wave * SUB_ROWS + r, a.m - 1)];
    for (int64_t g = wave * SUB_ROWS; g < a.m; g += step) {
        int64_t row[SUB_ROWS];
#pragma unroll
        for (int r = 0; r < SUB_ROWS; ++r) row[r] = next[r];   // (a short last group reads its last row again)
#pragma unroll
        for (int r = 0; r < SUB_ROWS; ++r) next[r] = a.ids[min(g + step + r, a.m - 1)];
        // norm and lambda of row `lane` of the group, in flight under the dot products (lanes 0 .. SUB_ROWS - 1)
        double nrm = 0.0, lam = 0.0;
        if (lane < SUB_ROWS) {
            const int64_t j = lane == 0 ? row[0] : lane == 1 ? row[1] : lane == 2 ? row[2] : row[3];
            nrm = a.n64[j];
            lam = a.lam64[j];
        }
        double acc[SUB_ROWS];
#pragma unroll
        for (int r = 0; r < SUB_ROWS; ++r) acc[r] = 0.0;
        if (F64) {
            constexpr int U = 6;   // 64 doubles per load of a wave: 384 columns of 4 rows before the first FMA
            for (int64_t base = 0; base < a.d; base += 64 * U) {
                double v[SUB_ROWS][U];
#pragma unroll
                for (int r = 0; r < SUB_ROWS; ++r) {
                    const double* pj = a.x64 + row[r] * a.d;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int64_t e = base + 64 * u + lane;
                        v[r][u] = e < a.d ? pj[e] : 0.0;
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t e = base + 64 * u + lane;
                    if (e < a.d) {
                        const double qv = QLDS ? qs[e] : a.q64[e];
#pragma unroll
                        for (int r = 0; r < SUB_ROWS; ++r) acc[r] += qv * v[r][u];
                    }
                }
            }
        } else {
            constexpr int U = 3;   // 256 floats per load of a wave: a whole 768-float row of 4 rows before the first FMA
            for (int64_t base = 0; base < a.dp; base += 256 * U) {
                f32x4 v[SUB_ROWS][U];
#pragma unroll
                for (int r = 0; r < SUB_ROWS; ++r) {
                    const float* pj = a.x32 + row[r] * a.dp;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int64_t e = base + 256 * u + 4 * lane;   // (dp is a multiple of 32: e < dp leaves 4 floats)
                        v[r][u] = e < a.dp ? *(const f32x4*)(pj + e) : f32x4{0, 0, 0, 0};
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t e = base + 256 * u + 4 * lane;
                    if (e < a.dp) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const double qv = QLDS ? qs[e + t] : a.q64[e + t];
#pragma unroll
                            for (int r = 0; r < SUB_ROWS; ++r) acc[r] += qv * (double)v[r][u][t];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < SUB_ROWS; ++r) acc[r] = wave_sum(acc[r]);   // (__shfl_xor butterfly: every lane holds the sums)
        if (lane < SUB_ROWS && g + lane < a.m) {
            const double dot = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
            const double den = sqrt(nrm * a.nq);
            const double c = den > 0.0 ? dot / den : 0.0;
            a.scores[g + lane] = blend_score(a.tau, c, a.lq, lam);   // lanes 0 .. 3: one 32-byte store
        }
    }
}
static_assert(SUB_ROWS == 4, "the lane selects of subset_score_kernel are written for four rows");

// ------------------------------------------------------------------ selection
// Key of the entry at position i: 96 bits, hi = the score's bits mapped so that a larger score is a larger number (NaN lowest,
// -0 as +0), lo = ~i (a smaller position is a larger number).  The k-th largest key T is found digit by digit, SEL_BITS bits a
// pass, most significant first: a pass counts the entries whose key agrees with T's digits so far by their next digit; the
// kernel of the NEXT pass starts by finding the digit that holds the remaining rank (every block alike, from the finished
// histogram).  Keys are distinct, so exactly k entries have key >= T.
constexpr int SEL_BITS = 12;
constexpr int SEL_BINS = 1 << SEL_BITS;
constexpr int SEL_PASSES = 96 / SEL_BITS;
constexpr int SEL_HIST_WORDS = SEL_PASSES * SEL_BINS + 64;   // + the counter of collected positions (its own 256 bytes)

struct SubsetSel {
    unsigned long long t_hi;   // T's digits found so far (the others zero)
    unsigned int t_lo;
    unsigned int krem;         // rank still to find among the entries that agree with them (1-based, from the top)
};

__device__ __forceinline__ unsigned long long sel_ord(double s) {
    if (s != s) return 0ull;
    if (s == 0.0) s = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(s);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
// digit p (0 = most significant) of the key hi:lo
__device__ __forceinline__ unsigned int sel_digit(unsigned long long hi, unsigned int lo, int p) {
    if (p <= 4) return (unsigned int)(hi >> (52 - 12 * p)) & 0xfffu;
    if (p == 5) return ((unsigned int)(hi & 0xfull) << 8) | (lo >> 24);
    return p == 6 ? (lo >> 12) & 0xfffu : lo & 0xfffu;
}
// the key agrees with T in its first p digits
__device__ __forceinline__ bool sel_match(unsigned long long hi, unsigned int lo, const SubsetSel& st, int p) {
    const int nb = 12 * p;
    const unsigned long long mh = nb >= 64 ? ~0ull : (nb == 0 ? 0ull : ~0ull << (64 - nb));
    const unsigned int ml = nb <= 64 ? 0u : ~0u << (96 - nb);
    return ((hi ^ st.t_hi) & mh) == 0ull && ((lo ^ st.t_lo) & ml) == 0u;
}
// T after pass p from T after pass p - 1 and pass p's finished histogram: by all 256 threads of a block
__device__ __forceinline__ SubsetSel sel_advance(SubsetSel st, const unsigned int* __restrict__ hist, int p) {
    __shared__ unsigned int wtot[4], r_dg, r_krem;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    unsigned int h[16], s = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        h[j] = hist[16 * t + j];
        s += h[j];
    }
    unsigned int sfx = s;   // inclusive suffix sum over the lanes: this thread's bins and the higher ones of its wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int v = __shfl_down(sfx, o, 64);
        if (lane + o < 64) sfx += v;
    }
    if (lane == 0) wtot[w] = sfx;
    if (t == 0) {
        r_dg = 0;
        r_krem = st.krem;
    }
    __syncthreads();
    unsigned int above = sfx - s;
    for (int u = w + 1; u < 4; ++u) above += wtot[u];
    if (above < st.krem && st.krem <= above + s) {   // the rank falls into this thread's 16 bins
        unsigned int acc = above;
        bool done = false;
#pragma unroll
        for (int j = 15; j >= 0; --j) {
            if (!done) {
                if (st.krem <= acc + h[j]) {
                    r_dg = 16 * t + j;
                    r_krem = st.krem - acc;
                    done = true;
                } else {
                    acc += h[j];
                }
            }
        }
    }
    __syncthreads();
    const unsigned int dg = r_dg;
    st.krem = r_krem;
    if (p <= 4) st.t_hi |= (unsigned long long)dg << (52 - 12 * p);
    else if (p == 5) {
        st.t_hi |= (unsigned long long)(dg >> 8);
        st.t_lo |= (dg & 0xffu) << 24;
    } else st.t_lo |= p == 6 ? dg << 12 : dg;
    return st;
}
// the state the kernel of pass p works with (p = SEL_PASSES: the collecting kernel): T's first p digits
__device__ __forceinline__ SubsetSel sel_state(int p, int k, SubsetSel* state, const unsigned int* hist) {
    SubsetSel st;
    st.t_hi = 0ull;
    st.t_lo = 0u;
    st.krem = (unsigned int)k;
    if (p == 0) return st;
    if (p > 1) st = state[p - 1];   // written by block 0 of the previous kernel
    st = sel_advance(st, hist + (int64_t)(p - 1) * SEL_BINS, p - 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) state[p] = st;
    return st;
}

__global__ __launch_bounds__(256) void subset_hist_kernel(const double* __restrict__ scores, int64_t m, int k, int p, SubsetSel* state,
                                                          unsigned int* hist) {
    __shared__ unsigned int lh[SEL_BINS];
    for (int b = threadIdx.x; b < SEL_BINS; b += blockDim.x) lh[b] = 0u;
    const SubsetSel st = sel_state(p, k, state, hist);   // (its barriers order the zeroing above, too)
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long hi = sel_ord(scores[i]);
        const unsigned int lo = ~(unsigned int)i;
        if (sel_match(hi, lo, st, p)) atomicAdd(&lh[sel_digit(hi, lo, p)], 1u);
    }
    __syncthreads();
    unsigned int* gh = hist + (int64_t)p * SEL_BINS;
    for (int b = threadIdx.x; b < SEL_BINS; b += blockDim.x)
        if (lh[b]) atomicAdd(&gh[b], lh[b]);
}

// the positions whose key is at or above T, in any order: exactly k of them
__global__ __launch_bounds__(256) void subset_collect_kernel(const double* __restrict__ scores, int64_t m, int k, SubsetSel* state,
                                                             unsigned int* hist, int32_t* sel_pos) {
    const SubsetSel st = sel_state(SEL_PASSES, k, state, hist);
    unsigned int* cnt = hist + (int64_t)SEL_PASSES * SEL_BINS;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long hi = sel_ord(scores[i]);
        const unsigned int lo = ~(unsigned int)i;
        if (hi > st.t_hi || (hi == st.t_hi && lo >= st.t_lo)) {
            const unsigned int slot = atomicAdd(cnt, 1u);
            if (slot < (unsigned int)SUBSET_TOPK) sel_pos[slot] = (int32_t)i;
        }
    }
}

// One block: the selected entries (sel_pos; null: all m <= SUBSET_TOPK positions) ranked by (score descending, position
// ascending) -- positions of a sorted id list are in id order --, the first k published to the pinned result.
__global__ __launch_bounds__(1024) void subset_sort_kernel(const double* __restrict__ scores, const int32_t* __restrict__ ids, int64_t m,
                                                           int k, const int32_t* __restrict__ sel_pos, const unsigned int* __restrict__ sel_cnt,
                                                           SubsetOut* out) {
    __shared__ unsigned long long sk[SUBSET_TOPK];
    __shared__ int32_t sp[SUBSET_TOPK];
    int n = sel_pos ? (int)(*sel_cnt < (unsigned int)SUBSET_TOPK ? *sel_cnt : (unsigned int)SUBSET_TOPK) : (int)m;
    if (n > SUBSET_TOPK) n = SUBSET_TOPK;
    const int t = threadIdx.x;
    double mys = 0.0;
    if (t < n) {
        const int32_t pos = sel_pos ? sel_pos[t] : t;
        mys = scores[pos];
        sk[t] = sel_ord(mys);
        sp[t] = pos;
    }
    __syncthreads();
    if (t < n) {
        const unsigned long long myk = sk[t];
        const int32_t myp = sp[t];
        int rank = 0;
        for (int s = 0; s < n; ++s) rank += (sk[s] > myk || (sk[s] == myk && sp[s] < myp)) ? 1 : 0;
        if (rank < k) {
            out->idx[rank] = ids[myp];
            out->score[rank] = mys;
        }
    }
    if (t == 0) out->len = n < k ? n : k;
}

// ------------------------------------------------------------------ host side
// |q|^2 as the search forms it (as_search.hip: q_prepare_kernel on the device, host_query_norm on the host -- 256 partial sums,
// element c in partial c % 256, products and sums rounded separately, then a pairwise tree): the same bits, so the cosines of
// the two routes share their denominator.  A third statement of that order (q_prepare_kernel points back here): whoever
// changes it there changes it here.  A drift would cost a last bit of the cosine, inside the 1e-12 the tests hold the two routes to.
static double subset_query_norm(const double* q, int64_t d) {
    double p[256];
    for (int t = 0; t < 256; ++t) p[t] = 0.0;
    for (int64_t c = 0; c < d; ++c) {
        volatile double sq = q[c] * q[c];
        p[c & 255] = p[c & 255] + sq;
    }
    for (int o = 128; o > 0; o >>= 1)
        for (int t = 0; t < o; ++t) p[t] += p[t + o];
    return p[0];
}

void subset_work_free(SubsetWork* w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    (void)hipFree(w->ids);
    (void)hipFree(w->scores);
    (void)hipFree(w->q64);
    (void)hipFree(w->hist);
    (void)hipFree(w->state);
    (void)hipFree(w->sel_pos);
    if (w->hq) (void)hipHostFree(w->hq);
    if (w->out) (void)hipHostFree(w->out);
    for (int i = 0; i < 2; ++i)
        if (w->ev[i]) (void)hipEventDestroy(w->ev[i]);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;
}

as_status subset_work_create(const as_space* sp, int64_t cap, SubsetWork** out) {
    *out = nullptr;
    SubsetWork* w = new (std::nothrow) SubsetWork();
    if (!w) {
        set_err("subset: out of host memory");
        return AS_ENOMEM;
    }
    w->device = sp->device;
    if (cap >= (int64_t)1 << 31) {   // positions are 32-bit (the selection's key, sel_pos)
        set_err("subset: %lld ids exceed the supported maximum of 2^31 - 1", (long long)cap);
        delete w;
        return AS_EUNSUPPORTED;
    }
    w->cap = std::max<int64_t>(cap, 1);
    w->dp = sp->dp;
    if (hipDeviceGetAttribute(&w->cus, hipDeviceAttributeMultiprocessorCount, sp->device) != hipSuccess || w->cus <= 0) w->cus = 256;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipMalloc((void**)&w->ids, sizeof(int32_t) * w->cap)) != hipSuccess ||
        (e = hipMalloc((void**)&w->scores, sizeof(double) * w->cap)) != hipSuccess ||
        (e = hipMalloc((void**)&w->q64, sizeof(double) * w->dp)) != hipSuccess ||
        (e = hipMalloc((void**)&w->hist, sizeof(unsigned int) * SEL_HIST_WORDS)) != hipSuccess ||
        (e = hipMalloc((void**)&w->state, sizeof(SubsetSel) * (SEL_PASSES + 1))) != hipSuccess ||
        (e = hipMalloc((void**)&w->sel_pos, sizeof(int32_t) * SUBSET_TOPK)) != hipSuccess ||
        (e = hipHostMalloc((void**)&w->hq, sizeof(double) * w->dp, hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc((void**)&w->out, sizeof(SubsetOut), hipHostMallocDefault)) != hipSuccess ||
        (e = hipEventCreate(&w->ev[0])) != hipSuccess || (e = hipEventCreate(&w->ev[1])) != hipSuccess) {
        set_err("subset: allocation of the work buffers (%lld ids) failed: %s", (long long)w->cap, hipGetErrorString(e));
        subset_work_free(w);
        return e == hipErrorOutOfMemory ? AS_ENOMEM : AS_EHIP;
    }
    for (int64_t c = 0; c < w->dp; ++c) w->hq[c] = 0.0;
    *out = w;
    return AS_OK;
}

as_status subset_set_ids(SubsetWork* w, const int32_t* ids_host, int64_t m) {
    if (m <= 0) return AS_OK;
    AS_HIP(hipMemcpyAsync(w->ids, ids_host, sizeof(int32_t) * m, hipMemcpyHostToDevice, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    return AS_OK;
}

// scores[i] = S11 score of item ids[i], i < m, queued on the work's stream (the query is uploaded in front of the kernel)
as_status subset_score(const as_space* sp, SubsetWork* w, int64_t m, const double* query, double tau, double lambda_q) {
    if (m <= 0) return AS_OK;
    for (int64_t c = 0; c < sp->d; ++c) w->hq[c] = query[c];   // (the pad stays zero)
    AS_HIP(hipMemcpyAsync(w->q64, w->hq, sizeof(double) * w->dp, hipMemcpyHostToDevice, w->stream));
    SubsetArgs a;
    a.ids = w->ids; a.m = m; a.x32 = sp->x32; a.x64 = sp->x64; a.n64 = sp->n64; a.lam64 = sp->lam64; a.q64 = w->q64;
    a.scores = w->scores; a.d = sp->d; a.dp = sp->dp; a.nq = subset_query_norm(query, sp->d); a.lq = lambda_q; a.tau = tau;
    const int64_t groups = (m + SUB_ROWS - 1) / SUB_ROWS;   // one per wave and trip
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((groups + 3) / 4, (int64_t)w->cus * SUB_BLOCKS_PER_CU));
    const bool qlds = sp->dp <= SUB_Q_LDS;
    const size_t lds = qlds ? sizeof(double) * (size_t)sp->dp : 0;
    if (w->timing) AS_HIP(hipEventRecord(w->ev[0], w->stream));
    if (sp->x64) {
        if (qlds) hipLaunchKernelGGL((subset_score_kernel<true, true>), dim3(grid), dim3(256), lds, w->stream, a);
        else hipLaunchKernelGGL((subset_score_kernel<true, false>), dim3(grid), dim3(256), 0, w->stream, a);
    } else {
        if (qlds) hipLaunchKernelGGL((subset_score_kernel<false, true>), dim3(grid), dim3(256), lds, w->stream, a);
        else hipLaunchKernelGGL((subset_score_kernel<false, false>), dim3(grid), dim3(256), 0, w->stream, a);
    }
    AS_HIP(hipGetLastError());
    if (w->timing) AS_HIP(hipEventRecord(w->ev[1], w->stream));
    return AS_OK;
}

static as_status subset_finish_timing(SubsetWork* w) {
    if (w->timing) {
        float ms = 0.0f;
        AS_HIP(hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
        w->kernel_us = (double)ms * 1e3;
    }
    return AS_OK;
}

// the first k of the m scores by (score descending, position ascending) -> ids and scores; waits for the stream
as_status subset_select(SubsetWork* w, int64_t m, int64_t k, int64_t* out_idx, double* out_score, int64_t* out_len) {
    *out_len = 0;
    if (m <= 0 || k <= 0) return AS_OK;
    k = std::min<int64_t>(std::min<int64_t>(k, m), SUBSET_TOPK);
    if (m <= SUBSET_TOPK) {
        hipLaunchKernelGGL(subset_sort_kernel, dim3(1), dim3(1024), 0, w->stream, (const double*)w->scores, (const int32_t*)w->ids, m, (int)k,
                           (const int32_t*)nullptr, (const unsigned int*)nullptr, w->out);
    } else {
        AS_HIP(hipMemsetAsync(w->hist, 0, sizeof(unsigned int) * SEL_HIST_WORDS, w->stream));
        const unsigned grid = (unsigned)std::min<int64_t>((m + 2047) / 2048, 512);
        for (int p = 0; p < SEL_PASSES; ++p)
            hipLaunchKernelGGL(subset_hist_kernel, dim3(grid), dim3(256), 0, w->stream, (const double*)w->scores, m, (int)k, p, w->state, w->hist);
        hipLaunchKernelGGL(subset_collect_kernel, dim3(grid), dim3(256), 0, w->stream, (const double*)w->scores, m, (int)k, w->state, w->hist,
                           w->sel_pos);
        hipLaunchKernelGGL(subset_sort_kernel, dim3(1), dim3(1024), 0, w->stream, (const double*)w->scores, (const int32_t*)w->ids, m, (int)k,
                           (const int32_t*)w->sel_pos, (const unsigned int*)(w->hist + (int64_t)SEL_PASSES * SEL_BINS), w->out);
    }
    AS_HIP(hipGetLastError());
    AS_HIP(hipStreamSynchronize(w->stream));
    AS_TRY(subset_finish_timing(w));
    const int64_t len = w->out->len;
    if (len != k) {
        set_err("subset: the selection returned %lld of %lld entries", (long long)len, (long long)k);
        return AS_EHIP;
    }
    for (int64_t t = 0; t < len; ++t) {
        out_idx[t] = w->out->idx[t];
        out_score[t] = w->out->score[t];
    }
    *out_len = len;
    return AS_OK;
}

// the m scores themselves, in the order of the ids; waits for the stream
as_status subset_scores_out(SubsetWork* w, int64_t m, double* out) {
    if (m > 0) AS_HIP(hipMemcpyAsync(out, w->scores, sizeof(double) * m, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    return m > 0 ? subset_finish_timing(w) : AS_OK;
}

}  // namespace as
