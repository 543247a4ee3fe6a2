// Per-query candidate lists: b queries, each with its own list of item ids.  One ragged launch scores
// every (query, item) pair of a chunk of queries (lists_score_kernel: the lists cut into segments of at most LISTS_R entries, a block
// per segment, the single-query kernel's row loop inside), one block per list selects its first k entries exactly
// (lists_select_kernel: a radix select over LDS histograms, then a rank of at most 1024 entries).
// Tau sweeps over the lists (section 5.13): lists_score_kernel over ListsTausArgs blends every cosine with up to TAU_GROUP taus,
// the selection runs a block per (list, tau) pair (lists_run_taus).
// Entry points: as_api.hip (as_score_lists_batch, as_search_lists_batch and their _taus forms).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <new>
#include <type_traits>

#include "as_common.hpp"
#include "as_gather.hpp"

namespace as {

constexpr int LISTS_WAVES = 4;        // waves per block
constexpr int LISTS_R = 64;           // entries per segment: staging a query (dp * 8 bytes) is 2 / R of the segment's fp32 row bytes (1 / R of fp64 rows)
constexpr int LISTS_BLOCKS_PER_CU = 4;
constexpr int64_t LISTS_QC_MAX = 4096;   // queries per chunk at most (the pinned results and the tables are sized by it)

struct ListsSeg {    // a work item of lists_score_kernel: 1 <= `count` <= LISTS_R consecutive entries of one list of the chunk
    int64_t first;   // entry of the chunk
    int32_t query;   // query of the chunk
    int32_t count;
};
struct ListsTausSeg {   // a segment that knows its list: list t of the chunk owns scores[nt * lfirst .. nt * (lfirst + len)) as [nt][len]
    int64_t first;      // entry of the chunk (the ids)
    int64_t lfirst;     // first entry of the segment's list
    int64_t len;        // entries of the segment's list
    int32_t query;
    int32_t count;
};
struct ListsList {   // a list of the chunk for lists_select_kernel
    int64_t first;
    int64_t len;     // 0: empty, or a query that is not served (lambda_q == 0)
};

struct ListsArgs {
    const ListsSeg* segs;
    int64_t nseg;
    const int32_t* ids;
    const float* x32;
    const double* x64;
    const double* n64;
    const double* lam64;
    const double* q64;   // [nb][dp] the chunk's queries, zero padded
    const double* nq;    // [nb] |q|^2
    const double* lq;    // [nb] lambda_q
    double* scores;      // [entries of the chunk]
    int64_t d, dp;
    double tau;
};
// The tau sweep's arguments (section 5.13): the taus and their count travel in the struct (scalar loads)
struct ListsTausArgs {
    ListsArgs s;        // (s.segs and s.tau are not read)
    const ListsTausSeg* segs;
    int nt;
    double taus[TAU_GROUP];
};

// A block takes segments grid-stride; per segment it stages the segment's query in LDS (QLDS; not again when the block's
// previous segment had the same one) and runs subset_score_kernel's row loop over the segment's rows: one wave per row,
// GATHER_ROWS rows at a time (gather_trip, as_gather.hpp), the ids wave-uniform and fetched one trip ahead.  A row's lane
// partition, accumulation order and butterfly are the same wherever its entry stands: the bits of a score depend on the query,
// the row, tau and lambda_q only (and equal the single form's for the same lambda_q).
// Args = ListsArgs: one score per entry, scores[entry]; ListsTausArgs: the cosine is formed once and blended with each of
// nt <= TAU_GROUP taus into the planes of the entry's list.  Everything in front of the stores is one body, so a plane holds
// the bits the single-tau instantiation writes for that tau.
template <bool F64, bool QLDS, class Args>
__global__ __launch_bounds__(256) void lists_score_kernel(Args args) {
    constexpr bool TAUS = std::is_same<Args, ListsTausArgs>::value;
    const ListsArgs* base;   // (picked in place: handing `args` to a helper by reference cost the fp32 instantiations up to 22 VGPRs)
    if constexpr (TAUS) base = &args.s;
    else base = &args;
    const ListsArgs& a = *base;
    extern __shared__ double qs[];
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    constexpr int64_t step = LISTS_WAVES * GATHER_ROWS;
    int staged = -1;
    for (int64_t s = blockIdx.x; s < a.nseg; s += gridDim.x) {
        const auto sg = args.segs[s];   // (ListsSeg or ListsTausSeg; s is uniform: scalar loads)
        const double* qg = a.q64 + (int64_t)sg.query * a.dp;
        if (QLDS && sg.query != staged) {
            __syncthreads();   // every wave has finished the previous segment's reads of qs
            for (int64_t c = threadIdx.x; c < a.dp; c += blockDim.x) qs[c] = qg[c];
            __syncthreads();
            staged = sg.query;
        }
        const double nqv = a.nq[sg.query], lqv = a.lq[sg.query];
        const int64_t end = sg.first + sg.count, last = end - 1;
        int64_t g = sg.first + (int64_t)w * GATHER_ROWS;
        int32_t next[GATHER_ROWS];
#pragma unroll
        for (int r = 0; r < GATHER_ROWS; ++r) next[r] = a.ids[min(g + r, last)];
        for (; g < end; g += step) {
            int64_t row[GATHER_ROWS];
#pragma unroll
            for (int r = 0; r < GATHER_ROWS; ++r) row[r] = next[r];   // (a short last group reads its last row again)
#pragma unroll
            for (int r = 0; r < GATHER_ROWS; ++r) next[r] = a.ids[min(g + step + r, last)];
            double nrm = 0.0, lam = 0.0;
            if (lane < GATHER_ROWS) {
                const int64_t j = lane == 0 ? row[0] : lane == 1 ? row[1] : lane == 2 ? row[2] : row[3];
                nrm = a.n64[j];
                lam = a.lam64[j];
            }
            double acc[GATHER_ROWS];
            gather_trip<F64, QLDS>(a.x32, a.x64, a.d, a.dp, row, qs, [&](int64_t e) { return qg[e]; }, lane, acc);
#pragma unroll
            for (int r = 0; r < GATHER_ROWS; ++r) acc[r] = wave_sum(acc[r]);
            if (lane < GATHER_ROWS && g + lane < end) {
                const double dot = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
                const double den = sqrt(nrm * nqv);
                const double c = den > 0.0 ? dot / den : 0.0;
                if constexpr (TAUS) {
                    // entry g + lane of the chunk is entry g + lane - lfirst of its list: plane j of the list's [nt][len] block
                    double* out = a.scores + (int64_t)args.nt * sg.lfirst + (g + lane - sg.lfirst);
#pragma unroll
                    for (int j = 0; j < TAU_GROUP; ++j)   // (unrolled: taus[j] is a scalar load, j < nt a scalar compare)
                        if (j < args.nt) out[j * sg.len] = blend_score(args.taus[j], c, lqv, lam);
                } else {
                    a.scores[g + lane] = blend_score(a.tau, c, lqv, lam);
                }
            }
        }
    }
}

// ------------------------------------------------------------------ selection
// Key of an entry: 96 bits, hi = the score's bits mapped so that a larger score is a larger number (sel_ord of as_common.hpp:
// NaN lowest, -0 as +0), lo = ~id: among equal scores the smaller index is the larger key, whatever the caller's
// order.  The ids of a list are distinct (the host removes duplicates), so no two keys of a list are equal.
constexpr int LSEL_NT = 256;
constexpr int LSEL_BINS = 4096;   // 12 bits a pass, most significant first
constexpr int LSEL_PASSES = 8;
constexpr int LSEL_CAP = 1024;    // entries the final rank takes (== SUBSET_TOPK >= k)
static_assert(LSEL_BINS == 16 * LSEL_NT && LSEL_CAP >= SUBSET_TOPK, "a thread owns 16 bins; the rank holds every requested entry");

struct ListsSelArgs {
    const ListsList* lists;
    const double* scores;
    const int32_t* ids;
    int64_t kk;          // entries asked for per list; the stride of out_idx / out_score
    int64_t* out_len;    // pinned [nb]
    int64_t* out_idx;    // pinned [nb][kk]
    double* out_score;
    int nt;              // PLANES: tau planes per list; the blocks are the (list, plane) pairs, results pinned [nb * nt](kk)
};

// One block per list, any length.  A list of more than LSEL_CAP entries: the digits of the k-th largest key T are found most
// significant first, each pass a histogram in LDS of the entries that agree with T's digits so far; the passes stop as soon as
// the entries at or above T's prefix (T's unknown digits zero) number at most LSEL_CAP -- after the last pass exactly k do.
// Then (every list) the entries with key >= T are collected in LDS and ranked; the first k go to the pinned result.
// PLANES (the tau sweep, section 5.13): block p serves plane p % nt of list p / nt: the scores are that plane of the list's
// [nt][len] block (lists_score_kernel over ListsTausArgs), the ids the list's, shared by its planes.
template <bool PLANES>
__global__ __launch_bounds__(LSEL_NT) void lists_select_kernel(ListsSelArgs a) {
    __shared__ unsigned int hist[LSEL_BINS];
    __shared__ unsigned long long sk[LSEL_CAP];
    __shared__ int32_t sid[LSEL_CAP], spos[LSEL_CAP];
    __shared__ unsigned int wtot[LSEL_NT / 64], r_dg, r_krem, r_cnt, s_n;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t li = PLANES ? (int64_t)blockIdx.x / a.nt : (int64_t)blockIdx.x;
    const ListsList L = a.lists[li];
    const int64_t m = L.len;
    if (m <= 0) {   // (uniform)
        if (t == 0) a.out_len[blockIdx.x] = 0;
        return;
    }
    const unsigned int k = (unsigned int)min(a.kk, m);
    const double* __restrict__ sc = PLANES ? a.scores + a.nt * L.first + ((int64_t)blockIdx.x - li * a.nt) * m : a.scores + L.first;
    const int32_t* __restrict__ id = a.ids + L.first;
    unsigned long long t_hi = 0ull;
    unsigned int t_lo = 0u;
    if (m > LSEL_CAP) {
        unsigned int krem = k;   // rank still to find among the entries that agree with T's digits (1-based, from the top)
        for (int p = 0; p < LSEL_PASSES; ++p) {
            for (int b = t; b < LSEL_BINS; b += LSEL_NT) hist[b] = 0u;
            __syncthreads();
            for (int64_t i = t; i < m; i += LSEL_NT) {
                const unsigned long long hi = sel_ord(sc[i]);
                const unsigned int lo = ~(unsigned int)id[i];
                if (sel_match(hi, lo, t_hi, t_lo, p)) atomicAdd(&hist[sel_digit(hi, lo, p)], 1u);
            }
            __syncthreads();
            // the bin that holds rank krem: thread t owns bins 16 t .. 16 t + 15 (sel_advance of as_subset.hip)
            unsigned int h[16], s = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                h[j] = hist[16 * t + j];
                s += h[j];
            }
            unsigned int sfx = s;   // inclusive suffix sum over the lanes
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned int v = __shfl_down(sfx, o, 64);
                if (lane + o < 64) sfx += v;
            }
            if (lane == 0) wtot[w] = sfx;
            if (t == 0) {
                r_dg = 0;
                r_krem = krem;
                r_cnt = 0;
            }
            __syncthreads();
            unsigned int above = sfx - s;
            for (int u = w + 1; u < LSEL_NT / 64; ++u) above += wtot[u];
            if (above < krem && krem <= above + s) {   // the rank falls into this thread's 16 bins
                unsigned int acc = above;
                bool done = false;
#pragma unroll
                for (int j = 15; j >= 0; --j) {
                    if (!done) {
                        if (krem <= acc + h[j]) {
                            r_dg = 16 * t + j;
                            r_krem = krem - acc;
                            r_cnt = h[j];
                            done = true;
                        } else {
                            acc += h[j];
                        }
                    }
                }
            }
            __syncthreads();
            const unsigned int dg = r_dg, cnt = r_cnt;
            krem = r_krem;
            if (p <= 4) t_hi |= (unsigned long long)dg << (52 - 12 * p);
            else if (p == 5) {
                t_hi |= (unsigned long long)(dg >> 8);
                t_lo |= (dg & 0xffu) << 24;
            } else t_lo |= p == 6 ? dg << 12 : dg;
            // k - krem entries lie above T's prefix, cnt agree with it
            if (k - krem + cnt <= (unsigned int)LSEL_CAP) break;   // (uniform)
        }
    }
    if (t == 0) s_n = 0u;
    __syncthreads();
    for (int64_t i = t; i < m; i += LSEL_NT) {
        const unsigned long long hi = sel_ord(sc[i]);
        const int32_t j = id[i];
        const unsigned int lo = ~(unsigned int)j;
        if (hi > t_hi || (hi == t_hi && lo >= t_lo)) {
            const unsigned int slot = atomicAdd(&s_n, 1u);
            if (slot < (unsigned int)LSEL_CAP) {
                sk[slot] = hi;
                sid[slot] = j;
                spos[slot] = (int32_t)i;
            }
        }
    }
    __syncthreads();
    const int n = (int)min(s_n, (unsigned int)LSEL_CAP);
    for (int e = t; e < n; e += LSEL_NT) {
        const unsigned long long myk = sk[e];
        const int32_t myi = sid[e];
        unsigned int rank = 0;
        for (int u = 0; u < n; ++u) rank += (sk[u] > myk || (sk[u] == myk && sid[u] < myi)) ? 1u : 0u;
        if (rank < k) {
            a.out_idx[blockIdx.x * a.kk + rank] = myi;
            a.out_score[blockIdx.x * a.kk + rank] = sc[spos[e]];
        }
    }
    if (t == 0) a.out_len[blockIdx.x] = (int64_t)min((unsigned int)n, k);
}

// ------------------------------------------------------------------ host side
static std::atomic<int> g_lists_timing{0};
static std::atomic<int> g_lists_budget_mib{256};
void set_lists_timing(int v) { g_lists_timing.store(v ? 1 : 0, std::memory_order_relaxed); }
void set_lists_budget_mib(int v) { g_lists_budget_mib.store(v > 0 ? v : 256, std::memory_order_relaxed); }
int64_t lists_budget_doubles() {
    return std::max<int64_t>(((int64_t)g_lists_budget_mib.load(std::memory_order_relaxed) << 20) / (int64_t)sizeof(double), 1);
}

as_status lists_select_launch(hipStream_t stream, const int64_t* lists, const double* scores, const int32_t* ids, int64_t kk, int64_t nb,
                              int64_t* out_len, int64_t* out_idx, double* out_score) {
    static_assert(sizeof(ListsList) == 2 * sizeof(int64_t), "a list is its (first, len) pair");
    ListsSelArgs s;
    s.lists = (const ListsList*)lists; s.scores = scores; s.ids = ids; s.kk = kk;
    s.out_len = out_len; s.out_idx = out_idx; s.out_score = out_score; s.nt = 1;
    hipLaunchKernelGGL(lists_select_kernel<false>, dim3((unsigned)nb), dim3(LSEL_NT), 0, stream, s);
    AS_HIP(hipGetLastError());
    return AS_OK;
}

struct ListsWork {
    int device = 0;
    hipStream_t stream = nullptr;
    int cus = 256;
    // one upload per chunk: [nb][dp] queries, [nb] |q|^2, [nb] lambda_q, the segments, the lists, the ids
    dev_buf<char> up_d;
    pin_buf<char> up_h;            // pinned staging of the same
    dev_buf<double> scores;        // the chunk's scores, entry by entry
    pin_buf<int64_t> out_len;      // pinned results of the selection: one length per list, entries at stride kk
    pin_buf<int64_t> out_idx;
    pin_buf<double> out_score;
    dev_events<2> ev;
    double kernel_us = 0.0;        // the score kernel summed over the chunks of the last timed call
};

void lists_work_free(ListsWork* w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;   // (the buffers and the events free themselves)
}

double lists_kernel_us(const ListsWork* w) { return w ? w->kernel_us : 0.0; }

static as_status lists_work_create(const as_space* sp, ListsWork** out) {
    ListsWork* w = new (std::nothrow) ListsWork();
    if (!w) {
        set_err("lists: out of host memory");
        return AS_ENOMEM;
    }
    w->device = sp->device;
    if (hipDeviceGetAttribute(&w->cus, hipDeviceAttributeMultiprocessorCount, sp->device) != hipSuccess || w->cus <= 0) w->cus = 256;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking)) != hipSuccess || (e = w->ev.create()) != hipSuccess) {
        set_err("lists: creation of the stream and events failed: %s", hipGetErrorString(e));
        lists_work_free(w);
        return AS_EHIP;
    }
    *out = w;
    return AS_OK;
}

// room for a chunk: `up` bytes of upload, ne scores, and for the selection nb lists of kk entries; each grown by half again
static as_status lists_reserve(ListsWork* w, size_t up, int64_t ne, int64_t nb, int64_t kk) {
    if (up > std::min(w->up_d.size(), w->up_h.size())) {
        AS_TRY(reserve_or_err(w->up_d, up + up / 2, "lists upload"));
        AS_TRY(reserve_or_err(w->up_h, up + up / 2, "lists pinned upload"));
    }
    if (ne > (int64_t)w->scores.size()) AS_TRY(reserve_or_err(w->scores, ne + ne / 2, "lists scores"));
    const int64_t out_q = w->out_len.size(), out_e = std::min(w->out_idx.size(), w->out_score.size());
    if (kk > 0 && (nb > out_q || nb * kk > out_e)) {
        const int64_t cq = std::max<int64_t>(nb + nb / 2, out_q), ce = std::max<int64_t>(cq * kk, w->out_idx.size());
        AS_TRY(reserve_or_err(w->out_len, cq, "lists pinned lengths"));
        AS_TRY(reserve_or_err(w->out_idx, ce, "lists pinned ids"));
        AS_TRY(reserve_or_err(w->out_score, ce, "lists pinned scores"));
    }
    return AS_OK;
}

as_status lists_run(const as_space* sp, const int32_t* ids, const int64_t* offs, const double* queries, int64_t b, const double* lq,
                    const int32_t* status, double tau, int64_t kk, int64_t* out_idx, double* out_score, int64_t* out_len,
                    double* out_scores, int64_t* counts) {
    const bool sel = kk > 0;
    if (sel)
        for (int64_t i = 0; i < b; ++i) out_len[i] = 0;
    if (b <= 0 || offs[b] == 0) return AS_OK;
    if (!sp->lists_ws) AS_TRY(lists_work_create(sp, &sp->lists_ws));
    ListsWork* w = sp->lists_ws;
    const int64_t d = sp->d, dp = sp->dp;
    const int64_t budget = std::max<int64_t>(((int64_t)g_lists_budget_mib.load(std::memory_order_relaxed) << 20) / (int64_t)sizeof(double), 1);
    const bool timing = g_lists_timing.load(std::memory_order_relaxed) != 0;
    const bool qlds = dp <= GATHER_Q_LDS;
    const size_t lds = qlds ? sizeof(double) * (size_t)dp : 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    w->kernel_us = 0.0;
    for (int64_t i0 = 0; i0 < b;) {
        // the chunk: queries i0 .. i1 - 1, as many as the budget holds scores for; a list longer than the budget is a chunk of its own
        int64_t i1 = i0, ne = 0;
        while (i1 < b && i1 - i0 < LISTS_QC_MAX) {
            const int64_t m = offs[i1 + 1] - offs[i1];
            if (i1 > i0 && ne + m > budget) break;
            ne += m;
            ++i1;
        }
        const int64_t nb = i1 - i0, base = offs[i0];
        if (ne == 0) {   // empty lists only
            i0 = i1;
            continue;
        }
        const auto t0 = now();
        const int64_t nseg_max = ne / LISTS_R + nb;
        const size_t q_bytes = sizeof(double) * (size_t)(nb * (dp + 2));
        const size_t seg_off = q_bytes, list_off = seg_off + sizeof(ListsSeg) * (size_t)nseg_max;
        const size_t ids_off = list_off + sizeof(ListsList) * (size_t)nb, up = ids_off + sizeof(int32_t) * (size_t)ne;
        AS_TRY(lists_reserve(w, up, ne, nb, kk));
        char* const up_h = w->up_h;
        char* const up_d = w->up_d;
        stage_queries((double*)up_h, queries, i0, nb, nb, d, dp, lq);
        ListsSeg* hseg = (ListsSeg*)(up_h + seg_off);
        ListsList* hlist = (ListsList*)(up_h + list_off);
        int64_t nseg = 0, pairs = 0;
        for (int64_t t = 0; t < nb; ++t) {
            const int64_t i = i0 + t, first = offs[i] - base, m = offs[i + 1] - offs[i];
            const bool served = status[i] != AS_EZEROLAMBDA;
            hlist[t].first = first;
            hlist[t].len = served ? m : 0;
            if (!served) continue;
            pairs += m;
            // ceil(m / R) segments of nearly equal length (a list of 100: 50 + 50, not 64 + 36: the blocks' shares stay even)
            const int64_t ns = (m + LISTS_R - 1) / LISTS_R;
            for (int64_t u = 0, o = 0; u < ns; ++u) {
                const int64_t cnt = m / ns + (u < m % ns ? 1 : 0);
                hseg[nseg].first = first + o;
                hseg[nseg].query = (int32_t)t;
                hseg[nseg].count = (int32_t)cnt;
                ++nseg;
                o += cnt;
            }
        }
        memcpy(up_h + ids_off, ids + base, sizeof(int32_t) * (size_t)ne);
        counts[2] += std::chrono::duration_cast<std::chrono::nanoseconds>(now() - t0).count();
        if (nseg > 0) {
            AS_HIP(hipMemcpyAsync(up_d, up_h, up, hipMemcpyHostToDevice, w->stream));
            ListsArgs a;
            a.segs = (const ListsSeg*)(up_d + seg_off); a.nseg = nseg; a.ids = (const int32_t*)(up_d + ids_off);
            a.x32 = sp->x32; a.x64 = sp->x64; a.n64 = sp->n64; a.lam64 = sp->lam64; a.q64 = (const double*)up_d;
            a.nq = a.q64 + nb * dp; a.lq = a.nq + nb; a.scores = w->scores; a.d = d; a.dp = dp; a.tau = tau;
            const unsigned grid = (unsigned)filtered_grid(std::min<int64_t>(nseg, (int64_t)w->cus * LISTS_BLOCKS_PER_CU));
            if (timing) AS_HIP(hipEventRecord(w->ev.e[0], w->stream));
            if (sp->x64) {
                if (qlds) hipLaunchKernelGGL((lists_score_kernel<true, true, ListsArgs>), dim3(grid), dim3(256), lds, w->stream, a);
                else hipLaunchKernelGGL((lists_score_kernel<true, false, ListsArgs>), dim3(grid), dim3(256), 0, w->stream, a);
            } else {
                if (qlds) hipLaunchKernelGGL((lists_score_kernel<false, true, ListsArgs>), dim3(grid), dim3(256), lds, w->stream, a);
                else hipLaunchKernelGGL((lists_score_kernel<false, false, ListsArgs>), dim3(grid), dim3(256), 0, w->stream, a);
            }
            AS_HIP(hipGetLastError());
            if (timing) AS_HIP(hipEventRecord(w->ev.e[1], w->stream));
            counts[0] += 1;
            counts[1] += pairs;
            if (sel) {
                ListsSelArgs s;
                s.lists = (const ListsList*)(up_d + list_off); s.scores = w->scores; s.ids = a.ids; s.kk = kk;
                s.out_len = w->out_len; s.out_idx = w->out_idx; s.out_score = w->out_score; s.nt = 1;
                hipLaunchKernelGGL(lists_select_kernel<false>, dim3((unsigned)nb), dim3(LSEL_NT), 0, w->stream, s);
                AS_HIP(hipGetLastError());
            } else {
                // one copy per run of served queries: the scores of a query that is not served stay unwritten
                AS_TRY(for_served_runs(status, i0, nb, [&](int64_t t, int64_t u) -> as_status {
                    const int64_t e0 = offs[i0 + t] - base, e1 = offs[i0 + u] - base;
                    if (e1 > e0)
                        AS_HIP(hipMemcpyAsync(out_scores + base + e0, w->scores + e0, sizeof(double) * (size_t)(e1 - e0), hipMemcpyDeviceToHost,
                                              w->stream));
                    return AS_OK;
                }));
            }
            AS_TRY(sync_add_elapsed(w->stream, timing, w->ev.e, &w->kernel_us));
            if (sel)
                for (int64_t t = 0; t < nb; ++t) {
                    const int64_t i = i0 + t, want = std::min<int64_t>(kk, hlist[t].len);
                    if (w->out_len[t] != want) {
                        set_err("lists: the selection returned %lld of %lld entries for query %lld", (long long)w->out_len[t], (long long)want,
                                (long long)i);
                        return AS_EHIP;
                    }
                    for (int64_t r = 0; r < want; ++r) {
                        out_idx[i * kk + r] = w->out_idx[t * kk + r];
                        out_score[i * kk + r] = w->out_score[t * kk + r];
                    }
                    out_len[i] = want;
                }
        }
        i0 = i1;
    }
    return AS_OK;
}

// The tau sweep (section 5.13): lists_run's chunks with ONE upload per chunk for all its tau groups, then per group of tg <= TAU_GROUP
// taus one gather (lists_score_kernel over ListsTausArgs) into the chunk's [list][tg][len] planes and either one selection block per (list,
// tau) pair or the copies out; one stream wait per (chunk, group).  tg of a chunk is the largest that fits the budget for the
// chunk's first list (a longer list further on ends the chunk), so a list too long for the budget is alone at tg = 1.
as_status lists_run_taus(const as_space* sp, const int32_t* ids, const int64_t* offs, const double* queries, int64_t b, const double* lq,
                         const int32_t* status, const double* taus, int64_t nt, const int64_t* row, int64_t ntau, int64_t kk, int64_t* out_idx,
                         double* out_score, int64_t* out_len, double* out_scores, int64_t* counts) {
    const bool sel = kk > 0;
    if (sel)
        for (int64_t p = 0; p < b * ntau; ++p) out_len[p] = 0;
    if (b <= 0 || nt <= 0 || offs[b] == 0) return AS_OK;
    if (!sp->lists_ws) AS_TRY(lists_work_create(sp, &sp->lists_ws));
    ListsWork* w = sp->lists_ws;
    const int64_t d = sp->d, dp = sp->dp;
    const int64_t budget = std::max<int64_t>(((int64_t)g_lists_budget_mib.load(std::memory_order_relaxed) << 20) / (int64_t)sizeof(double), 1);
    const bool timing = g_lists_timing.load(std::memory_order_relaxed) != 0;
    const bool qlds = dp <= GATHER_Q_LDS;
    const size_t lds = qlds ? sizeof(double) * (size_t)dp : 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    w->kernel_us = 0.0;
    for (int64_t i0 = 0; i0 < b;) {
        const int64_t m0 = std::max<int64_t>(offs[i0 + 1] - offs[i0], 1);
        const int64_t tg = std::max<int64_t>(std::min<int64_t>(std::min<int64_t>(nt, TAU_GROUP), budget / m0), 1);
        int64_t i1 = i0, ne = 0;
        while (i1 < b && (i1 - i0 + 1) * tg <= LISTS_QC_MAX) {
            const int64_t m = offs[i1 + 1] - offs[i1];
            if (i1 > i0 && (ne + m) * tg > budget) break;
            ne += m;
            ++i1;
        }
        const int64_t nb = i1 - i0, base = offs[i0];
        if (ne == 0) {   // empty lists only
            i0 = i1;
            continue;
        }
        const auto t0 = now();
        const int64_t nseg_max = ne / LISTS_R + nb;
        const size_t q_bytes = sizeof(double) * (size_t)(nb * (dp + 2));
        const size_t seg_off = q_bytes, list_off = seg_off + sizeof(ListsTausSeg) * (size_t)nseg_max;
        const size_t ids_off = list_off + sizeof(ListsList) * (size_t)nb, up = ids_off + sizeof(int32_t) * (size_t)ne;
        AS_TRY(lists_reserve(w, up, ne * tg, nb * tg, kk));
        char* const up_h = w->up_h;
        char* const up_d = w->up_d;
        stage_queries((double*)up_h, queries, i0, nb, nb, d, dp, lq);
        ListsTausSeg* hseg = (ListsTausSeg*)(up_h + seg_off);
        ListsList* hlist = (ListsList*)(up_h + list_off);
        int64_t nseg = 0, pairs = 0;
        for (int64_t t = 0; t < nb; ++t) {
            const int64_t i = i0 + t, first = offs[i] - base, m = offs[i + 1] - offs[i];
            const bool served = status[i] != AS_EZEROLAMBDA;
            hlist[t].first = first;
            hlist[t].len = served ? m : 0;
            if (!served) continue;
            pairs += m;
            const int64_t ns = (m + LISTS_R - 1) / LISTS_R;   // (lists_run's segments)
            for (int64_t u = 0, o = 0; u < ns; ++u) {
                const int64_t cnt = m / ns + (u < m % ns ? 1 : 0);
                hseg[nseg].first = first + o;
                hseg[nseg].lfirst = first;
                hseg[nseg].len = m;
                hseg[nseg].query = (int32_t)t;
                hseg[nseg].count = (int32_t)cnt;
                ++nseg;
                o += cnt;
            }
        }
        memcpy(up_h + ids_off, ids + base, sizeof(int32_t) * (size_t)ne);
        counts[3] += std::chrono::duration_cast<std::chrono::nanoseconds>(now() - t0).count();
        if (nseg > 0) {
            AS_HIP(hipMemcpyAsync(up_d, up_h, up, hipMemcpyHostToDevice, w->stream));
            ListsTausArgs a;
            a.s.segs = nullptr; a.s.nseg = nseg; a.s.ids = (const int32_t*)(up_d + ids_off);
            a.s.x32 = sp->x32; a.s.x64 = sp->x64; a.s.n64 = sp->n64; a.s.lam64 = sp->lam64; a.s.q64 = (const double*)up_d;
            a.s.nq = a.s.q64 + nb * dp; a.s.lq = a.s.nq + nb; a.s.scores = w->scores; a.s.d = d; a.s.dp = dp; a.s.tau = 0.0;
            a.segs = (const ListsTausSeg*)(up_d + seg_off);
            const unsigned grid = (unsigned)filtered_grid(std::min<int64_t>(nseg, (int64_t)w->cus * LISTS_BLOCKS_PER_CU));
            for (int64_t u0 = 0; u0 < nt; u0 += tg) {
                const int64_t g = std::min<int64_t>(tg, nt - u0);   // taus of this group: planes of every list's block
                a.nt = (int)g;
                for (int64_t j = 0; j < TAU_GROUP; ++j) a.taus[j] = j < g ? taus[u0 + j] : 0.0;
                if (timing) AS_HIP(hipEventRecord(w->ev.e[0], w->stream));
                if (sp->x64) {
                    if (qlds) hipLaunchKernelGGL((lists_score_kernel<true, true, ListsTausArgs>), dim3(grid), dim3(256), lds, w->stream, a);
                    else hipLaunchKernelGGL((lists_score_kernel<true, false, ListsTausArgs>), dim3(grid), dim3(256), 0, w->stream, a);
                } else {
                    if (qlds) hipLaunchKernelGGL((lists_score_kernel<false, true, ListsTausArgs>), dim3(grid), dim3(256), lds, w->stream, a);
                    else hipLaunchKernelGGL((lists_score_kernel<false, false, ListsTausArgs>), dim3(grid), dim3(256), 0, w->stream, a);
                }
                AS_HIP(hipGetLastError());
                if (timing) AS_HIP(hipEventRecord(w->ev.e[1], w->stream));
                counts[0] += 1;
                counts[1] += pairs;
                counts[2] += pairs * g;
                if (sel) {
                    ListsSelArgs s;
                    s.lists = (const ListsList*)(up_d + list_off); s.scores = w->scores; s.ids = a.s.ids; s.kk = kk;
                    s.out_len = w->out_len; s.out_idx = w->out_idx; s.out_score = w->out_score; s.nt = (int)g;
                    hipLaunchKernelGGL(lists_select_kernel<true>, dim3((unsigned)(nb * g)), dim3(LSEL_NT), 0, w->stream, s);
                    AS_HIP(hipGetLastError());
                } else if (g == ntau) {
                    // one group, no repeated tau: the device layout is the output's; one copy per run of served queries
                    AS_TRY(for_served_runs(status, i0, nb, [&](int64_t t, int64_t u) -> as_status {
                        const int64_t e0 = offs[i0 + t] - base, e1 = offs[i0 + u] - base;
                        if (e1 > e0)
                            AS_HIP(hipMemcpyAsync(out_scores + ntau * (base + e0), w->scores + g * e0, sizeof(double) * (size_t)((e1 - e0) * g),
                                                  hipMemcpyDeviceToHost, w->stream));
                        return AS_OK;
                    }));
                } else {
                    // per served query, one copy per run of planes whose output rows are consecutive
                    for (int64_t t = 0; t < nb; ++t) {
                        const int64_t m = hlist[t].len, first = hlist[t].first;
                        if (m == 0) continue;
                        for (int64_t j = 0; j < g;) {
                            int64_t j1 = j + 1;
                            while (j1 < g && row[u0 + j1] == row[u0 + j1 - 1] + 1) ++j1;
                            AS_HIP(hipMemcpyAsync(out_scores + ntau * (base + first) + row[u0 + j] * m, w->scores + g * first + j * m,
                                                  sizeof(double) * (size_t)((j1 - j) * m), hipMemcpyDeviceToHost, w->stream));
                            j = j1;
                        }
                    }
                }
                AS_TRY(sync_add_elapsed(w->stream, timing, w->ev.e, &w->kernel_us));
                if (sel)
                    for (int64_t t = 0; t < nb; ++t) {
                        const int64_t i = i0 + t, want = std::min<int64_t>(kk, hlist[t].len);
                        for (int64_t j = 0; j < g; ++j) {
                            const int64_t p = t * g + j, o = i * ntau + row[u0 + j];
                            if (w->out_len[p] != want) {
                                set_err("lists: the selection returned %lld of %lld entries for query %lld, tau %lld", (long long)w->out_len[p],
                                        (long long)want, (long long)i, (long long)row[u0 + j]);
                                return AS_EHIP;
                            }
                            for (int64_t r = 0; r < want; ++r) {
                                out_idx[o * kk + r] = w->out_idx[p * kk + r];
                                out_score[o * kk + r] = w->out_score[p * kk + r];
                            }
                            out_len[o] = want;
                        }
                    }
            }
        }
        i0 = i1;
    }
    return AS_OK;
}

}  // namespace as
