// Late-interaction re-ranking of per-need candidate documents: B needs of J_b query vectors, EACH WITH
// ITS OWN list of candidate groups ("documents").  The host expands every need's distinct documents into their members (item ids,
// by (label, id)); maxsim_lists_score_kernel scores every (vector, member) pair of a chunk of needs in ONE ragged launch: a work
// item is a segment of at most MSL_R consecutive entries of one need's expanded list under one TILE of that need's served vectors;
// the tile (as many vectors as fit GATHER_Q_LDS doubles, MSL_T_MAX at most) is staged in LDS and a wave forms the dots of
// GATHER_ROWS rows against every staged vector from one load of those rows.  Per (vector, row) the arithmetic is gather_trip's
// (as_gather.hpp) term by term: the same lane partition, one `acc += qv * v` per element in ascending e across the column chunks,
// the same butterfly, the same cosine and blend -- the bits are lists_score_kernel's (as_lists.hip) for the same lambda_q.
// maxsim_lists_fold_kernel: one wave per (need, document) takes, vector by vector, the maximum over the document's entries (NaN
// ignored, a zero maximum +0.0, NaN where every entry is NaN) and folds w_v x maximum by S13's step (as_fused_step.hpp): one double
// per (need, document), no atomics.  The lists' radix select (lists_select_kernel, unchanged) then names every need's first
// documents by (F descending, dense group number ascending == label ascending).  The J x E scores never leave the device.
// Entry points: as_api.hip (as_search_maxsim_lists, as_score_maxsim_lists, as_maxsim_lists_counters, as_maxsim_lists_kernel_us,
// as_maxsim_lists_geometry).
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), VGPRs of maxsim_lists_score_kernel<F64, QLDS,
// ONE>, none with scratch: fp64 <1,1,1> 125, <1,1,0> 123, <1,0,0> 94; fp32 <0,1,1> 118, <0,1,0> 127, <0,0,0> 124; the fold kernel 39:
// every instantiation stays at or under 128 VGPRs (4 waves per SIMD), as_gather.hpp's occupancy rule.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <limits>
#include <new>

#include "as_common.hpp"
#include "as_gather.hpp"

namespace as {

constexpr int MSL_WAVES = 4;           // waves per block
constexpr int MSL_R = 64;              // entries per segment (LISTS_R's reasoning: a staged tile is read for at least that many rows)
constexpr int MSL_T_MAX = 32;          // vectors per tile at most
constexpr int MSL_BLOCKS_PER_CU = 4;
constexpr int MSL_RUN = 4;             // consecutive work items a block takes per visit of its grid-stride loop, at most
constexpr int64_t MSL_NEEDS_MAX = 4096;   // needs per chunk at most (the selection's pinned results are sized by it)

int64_t maxsim_lists_tile(int64_t dp) { return dp <= GATHER_Q_LDS ? std::max<int64_t>(1, std::min<int64_t>(MSL_T_MAX, GATHER_Q_LDS / dp)) : 1; }
int64_t maxsim_lists_segment() { return MSL_R; }

struct MslSeg {       // a work item of the score kernel: 1 <= count <= MSL_R consecutive entries under 1 <= nvec <= T vectors
    int64_t first;    // entry of the chunk
    int64_t out;      // scores index of (vector vec0, entry first)
    int64_t stride;   // entries of the need's expanded list: vector v of the need owns scores[.. + v * stride ..]
    int32_t vec0;     // first vector of the tile among the chunk's served vectors
    int32_t nvec;
    int32_t count;
    int32_t pad;
};
struct MslDoc {       // a (need, document) of the chunk for the fold kernel
    int64_t first;    // scores index of (the need's first served vector, the document's first entry)
    int64_t stride;   // as MslSeg::stride
    int32_t count;    // entries (members) of the document
    int32_t vec0;     // the need's first served vector among the chunk's
    int32_t nvec;     // the need's served vectors (0: the need is not served)
    int32_t pad;
};

struct MslArgs {
    const MslSeg* segs;
    int64_t nseg;
    const int32_t* ids;
    const float* x32;
    const double* x64;
    const double* n64;
    const double* lam64;
    const double* q64;   // [nvs][dp] the chunk's served vectors, zero padded
    const double* nq;    // [nvs] |q|^2
    const double* lq;    // [nvs] lambda_q
    double* scores;
    int64_t d, dp;
    double tau;
    int run;             // consecutive work items a block takes per visit of its grid-stride loop
};

// The column chunk of gather_trip: U loads per row in flight before the first FMA (fp64: 64 doubles per load, fp32: 256 floats).
template <bool F64>
struct MslChunk;
template <>
struct MslChunk<true> {
    static constexpr int U = 6;
    static constexpr int64_t COLS = 64 * U;
    static constexpr int TV = 4;      // staged vectors whose dots a wave accumulates side by side: TV x GATHER_ROWS doubles
    typedef double elem;
};
template <>
struct MslChunk<false> {
    static constexpr int U = 3;
    static constexpr int64_t COLS = 256 * U;
    static constexpr int TV = 2;       // (4 costs the fp32 instantiations 150 and more VGPRs)
    typedef f32x4 elem;
};

// v <- the column chunk at `base` of the four rows: gather_trip's loads
template <bool F64>
__device__ __forceinline__ void msl_load(const float* x32, const double* x64, int64_t d, int64_t dp, const int64_t (&row)[GATHER_ROWS], int64_t base,
                                         int lane, typename MslChunk<F64>::elem (&v)[GATHER_ROWS][MslChunk<F64>::U]) {
    constexpr int U = MslChunk<F64>::U;
#pragma unroll
    for (int r = 0; r < GATHER_ROWS; ++r) {
        if constexpr (F64) {
            const double* pj = x64 + row[r] * d;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t e = base + 64 * u + lane;
                v[r][u] = e < d ? pj[e] : 0.0;
            }
        } else {
            const float* pj = x32 + row[r] * dp;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t e = base + 256 * u + 4 * lane;   // (dp is a multiple of 32: e < dp leaves 4 floats)
                v[r][u] = e < dp ? *(const f32x4*)(pj + e) : f32x4{0, 0, 0, 0};
            }
        }
    }
}

// The registers of a chunk are what they are, as far as the compiler can tell: without this it widens the 48 floats of four fp32
// rows to doubles ONCE in front of the loop over the vectors (96 registers) instead of beside each product.  No instruction.
template <bool F64>
__device__ __forceinline__ void msl_pin(typename MslChunk<F64>::elem (&v)[GATHER_ROWS][MslChunk<F64>::U]) {
#pragma unroll
    for (int r = 0; r < GATHER_ROWS; ++r)
#pragma unroll
        for (int u = 0; u < MslChunk<F64>::U; ++u) asm volatile("" : "+v"(v[r][u]));
}

// acc[t][r] += the lane's products of vector t (q + voff[t]: LDS or global memory) with the chunk of row r, gather_trip's order:
// u ascending, inside a 16-byte load t ascending, one `acc += qv * v` each.  nt <= TV vectors are live (wave-uniform).
template <bool F64, int TV>
__device__ __forceinline__ void msl_fma(const double* q, const int64_t (&voff)[TV], int nt, int64_t d, int64_t dp, int64_t base, int lane,
                                        const typename MslChunk<F64>::elem (&v)[GATHER_ROWS][MslChunk<F64>::U], double (&acc)[TV][GATHER_ROWS]) {
    constexpr int U = MslChunk<F64>::U;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if constexpr (F64) {
            const int64_t e = base + 64 * u + lane;
            if (e < d) {
#pragma unroll
                for (int t = 0; t < TV; ++t)
                    if (t == 0 || t < nt) {
                        const double qv = q[voff[t] + e];
#pragma unroll
                        for (int r = 0; r < GATHER_ROWS; ++r) acc[t][r] += qv * v[r][u];
                    }
            }
        } else {
            const int64_t e = base + 256 * u + 4 * lane;
            if (e < dp) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double x[GATHER_ROWS];
#pragma unroll
                    for (int r = 0; r < GATHER_ROWS; ++r) x[r] = (double)v[r][u][c];
                    // (no branch on t < nt here: a vector past the tile's last repeats vector t0 and is not stored; with the
                    // branch the widened elements stayed live across it and the instantiation went past 128 VGPRs)
#pragma unroll
                    for (int t = 0; t < TV; ++t) {
                        const double qv = q[voff[t] + e + c];
#pragma unroll
                        for (int r = 0; r < GATHER_ROWS; ++r) acc[t][r] += qv * x[r];
                    }
                }
            }
        }
    }
}

// A block takes work items grid-stride; per item it stages the item's tile of vectors in LDS (QLDS; not again when the block's
// previous item had the same tile) and walks the segment's rows as lists_score_kernel does: one wave per row, GATHER_ROWS rows at
// a time, the ids wave-uniform and fetched one trip ahead.  The rows' column chunk is loaded ONCE per trip where a row is one
// chunk (ONE; fp32: dp <= 768, fp64: d <= 384) and serves every staged vector, TV of them side by side in registers; a longer row
// is walked chunk by chunk once per TV vectors (the later walks hit the caches), so that a dot product's partial sums never
// leave their register and keep gather_trip's order.  !QLDS (dp > GATHER_Q_LDS): tiles of ONE vector, read from global memory.
// ONE (the host's choice: a row is one column chunk) is a template parameter: with both walks in one body the compiler kept the
// registers of both and every instantiation went past 128 VGPRs.
template <bool F64, bool QLDS, bool ONE>
__global__ __launch_bounds__(256) void maxsim_lists_score_kernel(MslArgs a) {
    constexpr int TV = QLDS ? MslChunk<F64>::TV : 1;
    constexpr int64_t COLS = MslChunk<F64>::COLS;
    extern __shared__ double qs[];
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    constexpr int64_t step = MSL_WAVES * GATHER_ROWS;
    const int64_t cols = F64 ? a.d : a.dp;
    int staged = -1;
    // (a block takes a.run consecutive work items per visit: they mostly share their tile, which is then staged once)
    for (int64_t s0 = (int64_t)blockIdx.x * a.run; s0 < a.nseg; s0 += (int64_t)gridDim.x * a.run) {
        const int64_t s1 = min(s0 + (int64_t)a.run, a.nseg);
        for (int64_t s = s0; s < s1; ++s) {
            const MslSeg sg = a.segs[s];   // (s is uniform: scalar loads)
            const double* qg = a.q64 + (int64_t)sg.vec0 * a.dp;
            if (QLDS && sg.vec0 != staged) {
                __syncthreads();   // every wave has finished the previous item's reads of qs
                const int64_t nq = (int64_t)sg.nvec * a.dp;
                for (int64_t c = threadIdx.x; c < nq; c += blockDim.x) qs[c] = qg[c];
                __syncthreads();
                staged = sg.vec0;
            }
            const double* q = QLDS ? qs : qg;
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
                typename MslChunk<F64>::elem v[GATHER_ROWS][MslChunk<F64>::U];
                if constexpr (ONE) msl_load<F64>(a.x32, a.x64, a.d, a.dp, row, 0, lane, v);
                for (int t0 = 0; t0 < sg.nvec; t0 += TV) {
                    const int nt = min(TV, sg.nvec - t0);
                    int64_t voff[TV];
#pragma unroll
                    for (int t = 0; t < TV; ++t) voff[t] = (int64_t)(t0 + (t < nt ? t : 0)) * a.dp;
                    double acc[TV][GATHER_ROWS];
#pragma unroll
                    for (int t = 0; t < TV; ++t)
#pragma unroll
                        for (int r = 0; r < GATHER_ROWS; ++r) acc[t][r] = 0.0;
                    if constexpr (ONE) {
                        msl_pin<F64>(v);
                        msl_fma<F64, TV>(q, voff, nt, a.d, a.dp, 0, lane, v, acc);
                    } else {
                        for (int64_t base = 0; base < cols; base += COLS) {
                            msl_load<F64>(a.x32, a.x64, a.d, a.dp, row, base, lane, v);
                            msl_fma<F64, TV>(q, voff, nt, a.d, a.dp, base, lane, v, acc);
                        }
                    }
#pragma unroll
                    for (int t = 0; t < TV; ++t)
                        if (t == 0 || t < nt) {
#pragma unroll
                            for (int r = 0; r < GATHER_ROWS; ++r) acc[t][r] = wave_sum(acc[t][r]);
                        }
                    if (lane < GATHER_ROWS && g + lane < end) {
                        double* out = a.scores + sg.out + (g + lane - sg.first);
#pragma unroll
                        for (int t = 0; t < TV; ++t)
                            if (t < nt) {
                                const int vec = sg.vec0 + t0 + t;
                                const double nqv = a.nq[vec], lqv = a.lq[vec];
                                const double dot = lane == 0 ? acc[t][0] : lane == 1 ? acc[t][1] : lane == 2 ? acc[t][2] : acc[t][3];
                                const double den = sqrt(nrm * nqv);
                                const double c = den > 0.0 ? dot / den : 0.0;
                                out[(int64_t)(t0 + t) * sg.stride] = blend_score(a.tau, c, lqv, lam);
                            }
                    }
                }
            }
        }
    }
}

}  // namespace as

#include "as_fused_step.hpp"   // fused_step; from here on nothing is contracted into an FMA

namespace as {

// the double a sel_ord key stands for (maxsim_decode of as_maxsim.hip): key 0 (nothing but NaN) is a NaN; -0.0 went in as +0.0
__device__ __forceinline__ double msl_decode(unsigned long long key) {
    if (key == 0ull) return __longlong_as_double(0x7ff8000000000000LL);
    const unsigned long long b = (key & 0x8000000000000000ull) ? (key & 0x7fffffffffffffffull) : ~key;
    return __longlong_as_double((long long)b);
}

// F[doc] <- the S13 sum over the need's served vectors, ascending, of w_v x the maximum of the document's entries under vector v.
// One wave per (need, document), documents grid-stride: the lanes share the entries, the maximum is one of sel_ord keys (exact in
// any order: NaN lowest, -0 as +0), every lane folds the same value.  A need that is not served (nvec == 0): NaN.
__global__ __launch_bounds__(64 * MSL_WAVES) void maxsim_lists_fold_kernel(const MslDoc* __restrict__ docs, int64_t ndoc,
                                                                          const double* __restrict__ scores, const double* __restrict__ wts,
                                                                          double* __restrict__ F) {
    const int lane = lane_id();
    const int64_t wv = (int64_t)blockIdx.x * MSL_WAVES + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * MSL_WAVES;
    for (int64_t dd = wv; dd < ndoc; dd += nw) {
        const MslDoc dc = docs[dd];
        double f = __longlong_as_double(0x7ff8000000000000LL);
        bool have = false;
        for (int j = 0; j < dc.nvec; ++j) {
            const double* __restrict__ s = scores + dc.first + (int64_t)j * dc.stride;
            unsigned long long k = 0ull;
            for (int i = lane; i < dc.count; i += 64) {
                const unsigned long long x = sel_ord(s[i]);
                k = x > k ? x : k;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long x = __shfl_xor(k, o, 64);
                k = x > k ? x : k;
            }
            f = fused_step<0>(f, wts[dc.vec0 + j], msl_decode(k), have);
            have = true;
        }
        if (lane == 0) F[dd] = f;
    }
}

// ------------------------------------------------------------------ host side
static std::atomic<int> g_maxsim_lists_timing{0};
void set_maxsim_lists_timing(int v) { g_maxsim_lists_timing.store(v ? 1 : 0, std::memory_order_relaxed); }

struct MaxsimListsWork {
    int device = 0;
    hipStream_t stream = nullptr;
    int cus = 256;
    // one upload per chunk: the served vectors ([nvs][dp], |q|^2, lambda_q, weights), the segments, the documents, the needs' document
    // ranges, the documents' dense group numbers, the ids
    dev_buf<char> up_d;
    pin_buf<char> up_h;
    dev_buf<double> scores;        // the chunk's scores: per need [served vectors][entries]
    dev_buf<double> F;             // one double per (need, document) of the chunk
    pin_buf<int64_t> out_len;      // pinned results of the selection: one length per need, entries at stride kk
    pin_buf<int64_t> out_idx;
    pin_buf<double> out_score;
    dev_events<4> ev;              // made by the first call under "maxsim_lists_timing": before the score kernel, behind it, behind the fold, behind the selection
};

void maxsim_lists_work_free(MaxsimListsWork* w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;   // (the buffers and the events free themselves)
}

static as_status maxsim_lists_work_create(const as_space* sp, MaxsimListsWork** out) {
    MaxsimListsWork* w = new (std::nothrow) MaxsimListsWork();
    if (!w) {
        set_err("maxsim lists: out of host memory");
        return AS_ENOMEM;
    }
    w->device = sp->device;
    if (hipDeviceGetAttribute(&w->cus, hipDeviceAttributeMultiprocessorCount, sp->device) != hipSuccess || w->cus <= 0) w->cus = 256;
    const hipError_t e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_err("maxsim lists: creation of the stream failed: %s", hipGetErrorString(e));
        maxsim_lists_work_free(w);
        return AS_EHIP;
    }
    *out = w;
    return AS_OK;
}

// room for a chunk, each part grown by half again: `up` bytes of upload, ns scores, nd documents, nb needs of kk entries
static as_status maxsim_lists_reserve(MaxsimListsWork* w, size_t up, int64_t ns, int64_t nd, int64_t nb, int64_t kk) {
    if (up > std::min(w->up_d.size(), w->up_h.size())) {
        AS_TRY(reserve_or_err(w->up_d, up + up / 2, "maxsim lists upload"));
        AS_TRY(reserve_or_err(w->up_h, up + up / 2, "maxsim lists pinned upload"));
    }
    if (ns > (int64_t)w->scores.size()) AS_TRY(reserve_or_err(w->scores, ns + ns / 2, "maxsim lists scores"));
    if (nd > (int64_t)w->F.size()) AS_TRY(reserve_or_err(w->F, nd + nd / 2, "maxsim lists document scores"));
    const int64_t out_q = w->out_len.size(), out_e = std::min(w->out_idx.size(), w->out_score.size());
    if (kk > 0 && (nb > out_q || nb * kk > out_e)) {
        const int64_t cq = std::max<int64_t>(nb + nb / 2, out_q), ce = std::max<int64_t>(cq * kk, w->out_idx.size());
        AS_TRY(reserve_or_err(w->out_len, cq, "maxsim lists pinned lengths"));
        AS_TRY(reserve_or_err(w->out_idx, ce, "maxsim lists pinned groups"));
        AS_TRY(reserve_or_err(w->out_score, ce, "maxsim lists pinned scores"));
    }
    return AS_OK;
}

static size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }

as_status maxsim_lists_run(const as_space* sp, const MaxsimListsIn& in, int64_t* out_gnum, double* out_score, int64_t* out_len, double* out_F,
                           int64_t* counts, double* us) {
    const bool sel = in.kk > 0;
    const int64_t b = in.b, kk = in.kk;
    if (sel)
        for (int64_t y = 0; y < b; ++y) out_len[y] = 0;
    us[0] = us[1] = us[2] = 0.0;
    if (b <= 0 || in.need_docs[b] == 0) return AS_OK;
    if (!sp->mlists_ws) AS_TRY(maxsim_lists_work_create(sp, &sp->mlists_ws));
    MaxsimListsWork* w = sp->mlists_ws;
    const int64_t d = sp->d, dp = sp->dp;
    const int64_t budget = lists_budget_doubles();
    const bool timing = g_maxsim_lists_timing.load(std::memory_order_relaxed) != 0;
    if (timing && !w->ev.e[3]) AS_HIP(w->ev.create());
    const bool qlds = dp <= GATHER_Q_LDS;
    const int64_t T = maxsim_lists_tile(dp);
    const size_t lds = qlds ? sizeof(double) * (size_t)(T * dp) : 0;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    auto now = [] { return std::chrono::steady_clock::now(); };
    // entries and served vectors of need y
    const auto entries = [&](int64_t y) { return in.doc_first[in.need_docs[y + 1]] - in.doc_first[in.need_docs[y]]; };
    const auto served = [&](int64_t y) {
        int64_t n = 0;
        if (in.nst[y] == 0)
            for (int64_t t = in.voffs[y]; t < in.voffs[y + 1]; ++t) n += in.vst[t] == AS_EZEROLAMBDA ? 0 : 1;
        return n;
    };
    for (int64_t i0 = 0; i0 < b;) {
        const auto t0 = now();
        // the chunk: needs i0 .. i1 - 1, as many as the budget holds scores for; a need larger than the budget is a chunk of its own
        int64_t i1 = i0, ns = 0, nvs = 0, nseg = 0;
        while (i1 < b && i1 - i0 < MSL_NEEDS_MAX) {
            const int64_t E = entries(i1), J = served(i1);
            if (i1 > i0 && ns + E * J > budget) break;
            ns += E * J;
            if (E > 0) {
                nvs += J;
                nseg += ((J + T - 1) / T) * ((E + MSL_R - 1) / MSL_R);
            }
            ++i1;
        }
        const int64_t nb = i1 - i0, dc0 = in.need_docs[i0], ndc = in.need_docs[i1] - dc0, e0 = in.doc_first[dc0], ne = in.doc_first[dc0 + ndc] - e0;
        if (ndc == 0) {   // empty lists only
            i0 = i1;
            continue;
        }
        const size_t q_bytes = sizeof(double) * (size_t)(nvs * (dp + 3));
        const size_t seg_off = q_bytes, doc_off = seg_off + sizeof(MslSeg) * (size_t)nseg, list_off = doc_off + sizeof(MslDoc) * (size_t)ndc;
        const size_t gnum_off = list_off + 2 * sizeof(int64_t) * (size_t)nb, ids_off = up8(gnum_off + sizeof(int32_t) * (size_t)ndc);
        const size_t up = ids_off + sizeof(int32_t) * (size_t)ne;
        AS_TRY(maxsim_lists_reserve(w, up, ns, ndc, nb, kk));
        char* const up_h = w->up_h;
        char* const up_d = w->up_d;
        double* hq = (double*)up_h;
        double* hn = hq + nvs * dp;
        double* hl = hn + nvs;
        double* hw = hl + nvs;
        MslSeg* hseg = (MslSeg*)(up_h + seg_off);
        MslDoc* hdoc = (MslDoc*)(up_h + doc_off);
        int64_t* hlist = (int64_t*)(up_h + list_off);   // (first, len) per need: lists_select_kernel's lists
        int32_t* hgnum = (int32_t*)(up_h + gnum_off);
        int64_t vs = 0, sg = 0, so = 0, pairs = 0, reads = 0;
        for (int64_t t = 0; t < nb; ++t) {
            const int64_t y = i0 + t, E = entries(y), dy0 = in.need_docs[y], dy1 = in.need_docs[y + 1], first = in.doc_first[dy0] - e0;
            const int64_t v0 = vs;
            if (in.nst[y] == 0 && E > 0)
                for (int64_t u = in.voffs[y]; u < in.voffs[y + 1]; ++u) {
                    if (in.vst[u] == AS_EZEROLAMBDA) continue;
                    const double* qv = in.queries + u * d;
                    double* rowq = hq + vs * dp;
                    for (int64_t c = 0; c < d; ++c) rowq[c] = qv[c];
                    for (int64_t c = d; c < dp; ++c) rowq[c] = 0.0;
                    hn[vs] = host_sumsq(qv, d);
                    hl[vs] = in.lq[u];
                    hw[vs] = in.wts[u];
                    ++vs;
                }
            const int64_t J = vs - v0;
            hlist[2 * t] = dy0 - dc0;
            hlist[2 * t + 1] = J > 0 ? dy1 - dy0 : 0;
            for (int64_t dd = dy0; dd < dy1; ++dd) {
                MslDoc& dc = hdoc[dd - dc0];
                dc.first = so + (in.doc_first[dd] - e0 - first);
                dc.stride = E;
                dc.count = (int32_t)(in.doc_first[dd + 1] - in.doc_first[dd]);
                dc.vec0 = (int32_t)v0;
                dc.nvec = (int32_t)J;
                dc.pad = 0;
                hgnum[dd - dc0] = in.doc_gnum[dd];
            }
            if (J == 0) continue;
            // per tile of vectors ceil(E / R) segments of nearly equal length (lists_run's split)
            const int64_t nsg = (E + MSL_R - 1) / MSL_R;
            // ceil(J / T) tiles of nearly equal size (8 vectors under T = 5: 4 + 4, not 5 + 3)
            const int64_t ntile = (J + T - 1) / T;
            for (int64_t ti = 0, tv = 0, nvec = 0; ti < ntile; ++ti, tv += nvec) {
                nvec = J / ntile + (ti < J % ntile ? 1 : 0);
                for (int64_t u = 0, o = 0; u < nsg; ++u) {
                    const int64_t cnt = E / nsg + (u < E % nsg ? 1 : 0);
                    MslSeg& s = hseg[sg++];
                    s.first = first + o;
                    s.out = so + tv * E + o;
                    s.stride = E;
                    s.vec0 = (int32_t)(v0 + tv);
                    s.nvec = (int32_t)nvec;
                    s.count = (int32_t)cnt;
                    s.pad = 0;
                    o += cnt;
                }
                reads += E;
            }
            pairs += E * J;
            so += E * J;
        }
        if (vs != nvs || sg != nseg || so != ns) {
            set_err("maxsim lists: the work tables of a chunk do not add up (%lld / %lld vectors, %lld / %lld segments, %lld / %lld scores)",
                    (long long)vs, (long long)nvs, (long long)sg, (long long)nseg, (long long)so, (long long)ns);
            return AS_EINVAL;
        }
        memcpy(up_h + ids_off, in.ids + e0, sizeof(int32_t) * (size_t)ne);
        counts[5] += std::chrono::duration_cast<std::chrono::nanoseconds>(now() - t0).count();
        if (nseg == 0) {   // no need of the chunk is served
            if (!sel) std::fill(out_F + dc0, out_F + dc0 + ndc, nan);
            i0 = i1;
            continue;
        }
        AS_HIP(hipMemcpyAsync(up_d, up_h, up, hipMemcpyHostToDevice, w->stream));
        MslArgs a;
        a.segs = (const MslSeg*)(up_d + seg_off); a.nseg = nseg; a.ids = (const int32_t*)(up_d + ids_off);
        a.x32 = sp->x32; a.x64 = sp->x64; a.n64 = sp->n64; a.lam64 = sp->lam64; a.q64 = (const double*)up_d;
        a.nq = a.q64 + nvs * dp; a.lq = a.nq + nvs; a.scores = w->scores; a.d = d; a.dp = dp; a.tau = in.tau;
        const double* dwts = a.lq + nvs;
        // runs of up to MSL_RUN items, shorter where the launch would otherwise leave compute units without a block
        const int64_t slots = (int64_t)w->cus * MSL_BLOCKS_PER_CU;
        a.run = (int)std::max<int64_t>(1, std::min<int64_t>(MSL_RUN, nseg / slots));
        const unsigned grid = (unsigned)filtered_grid(std::min<int64_t>((nseg + a.run - 1) / a.run, slots));
        if (timing) AS_HIP(hipEventRecord(w->ev.e[0], w->stream));
        // (a row that is one column chunk fits the staging as well: !qlds implies !one)
        if (sp->x64) {
            const bool one = d <= MslChunk<true>::COLS;
            if (one) hipLaunchKernelGGL((maxsim_lists_score_kernel<true, true, true>), dim3(grid), dim3(256), lds, w->stream, a);
            else if (qlds) hipLaunchKernelGGL((maxsim_lists_score_kernel<true, true, false>), dim3(grid), dim3(256), lds, w->stream, a);
            else hipLaunchKernelGGL((maxsim_lists_score_kernel<true, false, false>), dim3(grid), dim3(256), 0, w->stream, a);
        } else {
            const bool one = dp <= MslChunk<false>::COLS;
            if (one) hipLaunchKernelGGL((maxsim_lists_score_kernel<false, true, true>), dim3(grid), dim3(256), lds, w->stream, a);
            else if (qlds) hipLaunchKernelGGL((maxsim_lists_score_kernel<false, true, false>), dim3(grid), dim3(256), lds, w->stream, a);
            else hipLaunchKernelGGL((maxsim_lists_score_kernel<false, false, false>), dim3(grid), dim3(256), 0, w->stream, a);
        }
        AS_HIP(hipGetLastError());
        if (timing) AS_HIP(hipEventRecord(w->ev.e[1], w->stream));
        const unsigned fgrid = (unsigned)filtered_grid(std::min<int64_t>((ndc + MSL_WAVES - 1) / MSL_WAVES, (int64_t)w->cus * 8));
        double* F = w->F;
        hipLaunchKernelGGL(maxsim_lists_fold_kernel, dim3(fgrid), dim3(64 * MSL_WAVES), 0, w->stream, (const MslDoc*)(up_d + doc_off), ndc,
                           (const double*)w->scores, dwts, F);
        AS_HIP(hipGetLastError());
        if (timing) AS_HIP(hipEventRecord(w->ev.e[2], w->stream));
        counts[0] += nvs;
        counts[1] += 1;
        counts[2] += reads;
        counts[3] += pairs;
        counts[4] += 1;
        if (sel) {
            AS_TRY(lists_select_launch(w->stream, (const int64_t*)(up_d + list_off), F, (const int32_t*)(up_d + gnum_off), kk, nb, w->out_len,
                                       w->out_idx, w->out_score));
        } else {
            AS_HIP(hipMemcpyAsync(out_F + dc0, F, sizeof(double) * (size_t)ndc, hipMemcpyDeviceToHost, w->stream));
        }
        if (timing) AS_HIP(hipEventRecord(w->ev.e[3], w->stream));
        AS_HIP(hipStreamSynchronize(w->stream));
        if (timing)
            for (int t = 0; t < 3; ++t) {
                float ms = 0.0f;
                AS_HIP(hipEventElapsedTime(&ms, w->ev.e[t], w->ev.e[t + 1]));
                us[t] += (double)ms * 1e3;
            }
        if (sel)
            for (int64_t t = 0; t < nb; ++t) {
                const int64_t y = i0 + t, want = std::min<int64_t>(kk, hlist[2 * t + 1]);
                if (w->out_len[t] != want) {
                    set_err("maxsim lists: the selection returned %lld of %lld entries for need %lld", (long long)w->out_len[t], (long long)want,
                            (long long)y);
                    return AS_EHIP;
                }
                // entries that came back NaN lie behind the last document that has an answer
                int64_t n = 0;
                for (; n < want && w->out_score[t * kk + n] == w->out_score[t * kk + n]; ++n) {
                    out_gnum[y * kk + n] = w->out_idx[t * kk + n];
                    out_score[y * kk + n] = w->out_score[t * kk + n];
                }
                out_len[y] = n;
            }
        i0 = i1;
    }
    return AS_OK;
}

}  // namespace as
