// Diversified search (section 5.15): the greedy maximal-marginal-relevance pass over the hit list
// ("pool") an ordinary search returned.  One block per query runs the whole greedy in ONE launch (diverse_select_kernel): per
// step a block argmax over the margins of the unselected pool entries, then the cosines of the unselected rows with the row just
// picked -- the score kernels' four-row trip (gather_trip, as_gather.hpp) with the picked row in the query's place.  No P x P
// matrix is formed.
// Entry points: as_api.hip (as_search_diverse, as_search_diverse_batch).
#include <algorithm>
#include <atomic>
#include <new>

#include "as_common.hpp"
#include "as_gather.hpp"

namespace as {

constexpr int DIV_WAVES = 16;        // waves per block: 64 rows per trip (section 5.15: 1024 threads against 256, measured)
constexpr int DIV_POOL = SUBSET_TOPK;   // entries of a pool at most (== MAX_TOPK)
constexpr int64_t DIV_QC_DEFAULT = 4096;   // queries per chunk ("diverse_chunk")

struct DiverseArgs {
    const double* sc;      // [nq][kk] the pools' scores, position by position
    const int32_t* ids;    // [nq][kk] the pools' item ids
    const int32_t* plen;   // [nq] entries of each pool; 0: a query that is not served
    const float* x32;
    const double* x64;
    const double* n64;
    double* out_margin;    // [nq][nn] the margin pick t was made with
    int32_t* out_pos;      // [nq][nn] the pool position of pick t
    int64_t d, dp;
    int kk, nn;            // stride of the pools, picks wanted per query (its stride of the outputs)
    double delta;
};

// (margin descending, position ascending): a is ahead of b
__device__ __forceinline__ bool div_ahead(double ma, int pa, double mb, int pb) { return ma > mb || (ma == mb && pa < pb); }

// One block of DIV_WAVES waves per query.  LDS: the picked row as fp64 (QLDS), then per pool position its score s, the largest cosine r
// with a picked row and its item id, then `live`, the positions still unselected (a pick is replaced by the last entry: their order
// carries no meaning, the tie rule is part of the reduction key), then a slot per wave for the argmax.
// Step t: every thread folds the margins (1 - delta) s - delta r of live entries t, t + NT, ... (a NaN margin is -inf), a butterfly per
// wave and a pass over the waves' slots give every thread the same winner; then (not after the last pick) the winner's row is staged
// and the score kernels' trip (gather_trip, as_gather.hpp) runs over the live rows: one wave per row, GATHER_ROWS rows at a time.
// Lane partition, accumulation order and butterfly are lists_score_kernel's, and do not depend on which of the two rows is
// staged (every product is one multiply of the same two values): g(i, j) and g(j, i) have the same bits.
template <bool F64, bool QLDS>
__global__ __launch_bounds__(DIV_WAVES * 64) void diverse_select_kernel(DiverseArgs a) {
    extern __shared__ double dsm[];
    constexpr int WAVES = DIV_WAVES, NT = WAVES * 64;
    double* const qs = dsm;
    double* const s = dsm + (QLDS ? a.dp : 0);
    double* const r = s + a.kk;
    double* const wm = r + a.kk;
    int32_t* const id = (int32_t*)(wm + WAVES);
    int32_t* const live = id + a.kk;
    int32_t* const wp = live + a.kk;
    int32_t* const wk = wp + WAVES;
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t q = blockIdx.x;
    const int P = min(a.plen[q], a.kk);   // (q is uniform: a scalar load)
    if (P <= 0) return;                   // (uniform)
    const int nn = min(a.nn, P);
    for (int p = threadIdx.x; p < P; p += NT) {
        s[p] = a.sc[q * a.kk + p];
        r[p] = 0.0;
        id[p] = a.ids[q * a.kk + p];
        live[p] = p;
    }
    __syncthreads();
    const double ninf = -key_traits<double>::inf();
    const double om = 1.0 - a.delta;
    constexpr int step = WAVES * GATHER_ROWS;
    for (int t = 0; t < nn; ++t) {
        const int L = P - t;   // live entries
        double bm = ninf;
        int bp = 0x7fffffff, bk = 0;
        for (int k = threadIdx.x; k < L; k += NT) {
            const int p = live[k];
            double m = om * s[p] - a.delta * r[p];
            if (m != m) m = ninf;
            if (div_ahead(m, p, bm, bp)) {
                bm = m;
                bp = p;
                bk = k;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double xm = __shfl_xor(bm, o, 64);
            const int xp = __shfl_xor(bp, o, 64), xk = __shfl_xor(bk, o, 64);
            if (div_ahead(xm, xp, bm, bp)) {
                bm = xm;
                bp = xp;
                bk = xk;
            }
        }
        if (lane == 0) {
            wm[w] = bm;
            wp[w] = bp;
            wk[w] = bk;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < WAVES; ++u) {   // (the same address in every lane: broadcast reads)
            const double xm = wm[u];
            const int xp = wp[u], xk = wk[u];
            if (div_ahead(xm, xp, bm, bp)) {
                bm = xm;
                bp = xp;
                bk = xk;
            }
        }
        if (threadIdx.x == 0) {
            a.out_pos[q * a.nn + t] = bp;
            a.out_margin[q * a.nn + t] = bm;
        }
        if (t + 1 == nn) break;   // (uniform) the last pick: no cosine is needed any more
        __syncthreads();          // every thread has read live[] and the waves' slots
        if (threadIdx.x == 0) live[bk] = live[L - 1];
        const int64_t jsel = __builtin_amdgcn_readfirstlane(id[bp]);
        const double nsel = a.n64[jsel];
        const double* qg = a.x64 + jsel * a.d;    // (read where F64 only)
        const float* qf = a.x32 + jsel * a.dp;    // (read where !F64 only)
        if (QLDS) {
            for (int64_t c = threadIdx.x; c < a.dp; c += NT) qs[c] = F64 ? (c < a.d ? qg[c] : 0.0) : (double)qf[c];
        }
        __syncthreads();
        const int end = L - 1, last = end - 1;   // (end >= 1: t + 1 < nn <= P)
        for (int g = w * GATHER_ROWS; g < end; g += step) {
            int64_t row[GATHER_ROWS];
#pragma unroll
            for (int rr = 0; rr < GATHER_ROWS; ++rr) row[rr] = __builtin_amdgcn_readfirstlane(id[live[min(g + rr, last)]]);   // (a short last group reads its last row again)
            double nrm = 0.0;
            int pos = 0;
            if (lane < GATHER_ROWS && g + lane < end) {
                pos = live[g + lane];
                nrm = a.n64[id[pos]];
            }
            double acc[GATHER_ROWS];
            gather_trip<F64, QLDS>(a.x32, a.x64, a.d, a.dp, row, qs, [&](int64_t e) { return F64 ? qg[e] : (double)qf[e]; }, lane, acc);
#pragma unroll
            for (int rr = 0; rr < GATHER_ROWS; ++rr) acc[rr] = wave_sum(acc[rr]);
            if (lane < GATHER_ROWS && g + lane < end) {
                const double dot = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
                const double den = sqrt(nrm * nsel);
                const double c = den > 0.0 ? dot / den : 0.0;
                // the largest cosine with a picked row: the first pick sets it, negative values included
                r[pos] = (t == 0 || c > r[pos]) ? c : r[pos];
            }
        }
        __syncthreads();   // r is complete; every wave has finished its reads of qs and live[]
    }
}

// ------------------------------------------------------------------ host side
static std::atomic<int> g_diverse_timing{0};
static std::atomic<int64_t> g_diverse_chunk{DIV_QC_DEFAULT};
void set_diverse_timing(int v) { g_diverse_timing.store(v ? 1 : 0, std::memory_order_relaxed); }
void set_diverse_chunk(int v) { g_diverse_chunk.store(v > 0 ? v : DIV_QC_DEFAULT, std::memory_order_relaxed); }

struct DiverseWork {
    int device = 0;
    hipStream_t stream = nullptr;
    // one upload per chunk: [nb][kk] scores, [nb][kk] ids, [nb] pool lengths; one download: [nb][nn] margins, [nb][nn] positions
    dev_buf<char> up_d, out_d;
    pin_buf<char> up_h, out_h;
    dev_events<2> ev;
    double kernel_us = 0.0;   // the kernel summed over the chunks of the last timed call
};

void diverse_work_free(DiverseWork* w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;   // (the buffers and the events free themselves)
}

double diverse_kernel_us(const DiverseWork* w) { return w ? w->kernel_us : 0.0; }

static as_status diverse_work_create(const as_space* sp, DiverseWork** out) {
    DiverseWork* w = new (std::nothrow) DiverseWork();
    if (!w) {
        set_err("diverse: out of host memory");
        return AS_ENOMEM;
    }
    w->device = sp->device;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking)) != hipSuccess || (e = w->ev.create()) != hipSuccess) {
        set_err("diverse: creation of the stream and events failed: %s", hipGetErrorString(e));
        diverse_work_free(w);
        return AS_EHIP;
    }
    *out = w;
    return AS_OK;
}

// room for a chunk: `up` bytes of upload, `dn` of download; each grown by half again
static as_status diverse_reserve(DiverseWork* w, size_t up, size_t dn) {
    if (up > std::min(w->up_d.size(), w->up_h.size())) {
        AS_TRY(reserve_or_err(w->up_d, up + up / 2, "diverse upload"));
        AS_TRY(reserve_or_err(w->up_h, up + up / 2, "diverse pinned upload"));
    }
    if (dn > std::min(w->out_d.size(), w->out_h.size())) {
        AS_TRY(reserve_or_err(w->out_d, dn + dn / 2, "diverse results"));
        AS_TRY(reserve_or_err(w->out_h, dn + dn / 2, "diverse pinned results"));
    }
    return AS_OK;
}

as_status diverse_run(const as_space* sp, const int64_t* pool_idx, const double* pool_score, const int64_t* pool_len, int64_t kk, int64_t b,
                      int64_t n, double delta, int64_t* out_idx, double* out_score, double* out_margin, int64_t* out_len, int64_t* counts) {
    for (int64_t i = 0; i < b; ++i) out_len[i] = 0;
    const int64_t nn = std::min<int64_t>(n, kk);
    if (b <= 0 || nn <= 0) return AS_OK;
    if (kk > DIV_POOL) {
        set_err("diverse: a pool of %lld entries exceeds the supported maximum of %d", (long long)kk, DIV_POOL);
        return AS_EUNSUPPORTED;
    }
    // what the kernel gathers by: every id an item of this space, every length within the stride
    for (int64_t i = 0; i < b; ++i) {
        if (pool_len[i] < 0 || pool_len[i] > kk) {
            set_err("diverse: the pool of query %lld has %lld entries, at most %lld were asked for", (long long)i, (long long)pool_len[i], (long long)kk);
            return AS_EHIP;
        }
        for (int64_t p = 0; p < pool_len[i]; ++p)
            if (pool_idx[i * kk + p] < 0 || pool_idx[i * kk + p] >= sp->n) {
                set_err("diverse: the pool of query %lld holds id %lld outside [0, %lld)", (long long)i, (long long)pool_idx[i * kk + p], (long long)sp->n);
                return AS_EHIP;
            }
    }
    if (!sp->diverse_ws) AS_TRY(diverse_work_create(sp, &sp->diverse_ws));
    DiverseWork* w = sp->diverse_ws;
    const int64_t d = sp->d, dp = sp->dp;
    const int64_t chunk = g_diverse_chunk.load(std::memory_order_relaxed);
    const bool timing = g_diverse_timing.load(std::memory_order_relaxed) != 0;
    const bool qlds = dp <= GATHER_Q_LDS;
    const size_t lds = sizeof(double) * (size_t)((qlds ? dp : 0) + 2 * kk + DIV_WAVES) + sizeof(int32_t) * (size_t)(2 * kk + 2 * DIV_WAVES);
    w->kernel_us = 0.0;
    for (int64_t i0 = 0; i0 < b; i0 += chunk) {
        const int64_t nb = std::min<int64_t>(chunk, b - i0);
        int64_t served = 0;
        for (int64_t t = 0; t < nb; ++t) served += pool_len[i0 + t] > 0 ? 1 : 0;
        if (served == 0) continue;
        const size_t ids_off = sizeof(double) * (size_t)(nb * kk), len_off = ids_off + sizeof(int32_t) * (size_t)(nb * kk);
        const size_t up = len_off + sizeof(int32_t) * (size_t)nb;
        const size_t pos_off = sizeof(double) * (size_t)(nb * nn), dn = pos_off + sizeof(int32_t) * (size_t)(nb * nn);
        AS_TRY(diverse_reserve(w, up, dn));
        char* const up_h = w->up_h;
        char* const up_d = w->up_d;
        char* const out_h = w->out_h;
        char* const out_d = w->out_d;
        double* hs = (double*)up_h;
        int32_t* hid = (int32_t*)(up_h + ids_off);
        int32_t* hlen = (int32_t*)(up_h + len_off);
        for (int64_t t = 0; t < nb; ++t) {
            const int64_t i = i0 + t, m = pool_len[i];
            hlen[t] = (int32_t)m;
            for (int64_t p = 0; p < kk; ++p) {
                hs[t * kk + p] = p < m ? pool_score[i * kk + p] : 0.0;
                hid[t * kk + p] = p < m ? (int32_t)pool_idx[i * kk + p] : 0;
            }
            const int64_t k = std::min<int64_t>(nn, m);
            counts[1] += k;
            counts[2] += k > 0 ? (k - 1) * m - k * (k - 1) / 2 : 0;   // step t >= 1 forms m - t cosines
        }
        AS_HIP(hipMemcpyAsync(up_d, up_h, up, hipMemcpyHostToDevice, w->stream));
        DiverseArgs a;
        a.sc = (const double*)up_d; a.ids = (const int32_t*)(up_d + ids_off); a.plen = (const int32_t*)(up_d + len_off);
        a.x32 = sp->x32; a.x64 = sp->x64; a.n64 = sp->n64; a.out_margin = (double*)out_d; a.out_pos = (int32_t*)(out_d + pos_off);
        a.d = d; a.dp = dp; a.kk = (int)kk; a.nn = (int)nn; a.delta = delta;
        if (timing) AS_HIP(hipEventRecord(w->ev.e[0], w->stream));
        const dim3 grid((unsigned)nb), block(DIV_WAVES * 64);
        if (sp->x64) {
            if (qlds) hipLaunchKernelGGL((diverse_select_kernel<true, true>), grid, block, lds, w->stream, a);
            else hipLaunchKernelGGL((diverse_select_kernel<true, false>), grid, block, lds, w->stream, a);
        } else {
            if (qlds) hipLaunchKernelGGL((diverse_select_kernel<false, true>), grid, block, lds, w->stream, a);
            else hipLaunchKernelGGL((diverse_select_kernel<false, false>), grid, block, lds, w->stream, a);
        }
        AS_HIP(hipGetLastError());
        if (timing) AS_HIP(hipEventRecord(w->ev.e[1], w->stream));
        counts[0] += 1;
        AS_HIP(hipMemcpyAsync(out_h, out_d, dn, hipMemcpyDeviceToHost, w->stream));
        AS_TRY(sync_add_elapsed(w->stream, timing, w->ev.e, &w->kernel_us));
        const double* hm = (const double*)out_h;
        const int32_t* hp = (const int32_t*)(out_h + pos_off);
        for (int64_t t = 0; t < nb; ++t) {
            const int64_t i = i0 + t, m = pool_len[i], k = std::min<int64_t>(nn, m);
            for (int64_t u = 0; u < k; ++u) {
                const int64_t p = hp[t * nn + u];
                if (p < 0 || p >= m) {
                    set_err("diverse: pick %lld of query %lld is position %lld of a pool of %lld", (long long)u, (long long)i, (long long)p, (long long)m);
                    return AS_EHIP;
                }
                out_idx[i * nn + u] = pool_idx[i * kk + p];
                out_score[i * nn + u] = pool_score[i * kk + p];
                if (out_margin) out_margin[i * nn + u] = hm[t * nn + u];
            }
            out_len[i] = k;
        }
    }
    return AS_OK;
}

}  // namespace as
