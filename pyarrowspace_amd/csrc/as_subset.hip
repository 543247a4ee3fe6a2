// Filtered search: the exact S11 scores of a list of items gathered by id (subset_score_kernel) and the
// exact top-k of them by (score descending, position ascending) -- a radix select over an order-preserving 96-bit key (the
// score's bits, then the inverted position: no two keys are equal), then a one-block sort of the k selected entries.
// Entry points: as_api.hip (as_search_subset, as_score_items; the batched forms, section 5.10; the tau sweeps, section 5.11).
#include <algorithm>
#include <atomic>
#include <new>
#include <type_traits>

#include "as_common.hpp"
#include "as_gather.hpp"

namespace as {

constexpr int SUB_BLOCKS_PER_CU = 4;   // 4 blocks of 4 waves: 16 waves per CU

static std::atomic<int> g_filtered_grid_cap{0};
void set_filtered_grid_cap(int v) { g_filtered_grid_cap.store(v > 0 ? v : 0, std::memory_order_relaxed); }
int64_t filtered_grid(int64_t blocks) {
    const int64_t cap = g_filtered_grid_cap.load(std::memory_order_relaxed);
    return cap > 0 ? std::min<int64_t>(blocks, cap) : blocks;
}

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
// The tau sweep's arguments: the taus and their count travel in the struct (scalar loads)
struct SubsetTausArgs {
    SubsetArgs s;   // (s.tau is not read)
    int64_t ld;     // plane j: scores + j * ld
    int nt;
    double taus[TAU_GROUP];
};

// One wave per row, GATHER_ROWS rows at a time (gather_trip, as_gather.hpp), grid-stride over the id list; the ids are
// wave-uniform.  F64: the rows are the fp64 items, else the fp32 items; QLDS: the query is staged in LDS once per block.
// Args = SubsetArgs: one score per item; SubsetTausArgs: the cosine of a (query, item) pair is formed once and blended with
// each of nt <= TAU_GROUP taus into the planes scores[j * ld + pos].  Everything in front of the stores is one body, so for the
// same lambda_q a plane holds the bits the single-tau instantiation of the same route writes for that tau.
template <bool F64, bool QLDS, class Args>
__global__ __launch_bounds__(256) void subset_score_kernel(Args args) {
    constexpr bool TAUS = std::is_same<Args, SubsetTausArgs>::value;
    const SubsetArgs* base;   // (picked in place, not by a helper that takes `args` by reference: as_lists.hip)
    if constexpr (TAUS) base = &args.s;
    else base = &args;
    const SubsetArgs& a = *base;
    extern __shared__ double qs[];
    if (QLDS) {
        for (int64_t c = threadIdx.x; c < a.dp; c += blockDim.x) qs[c] = a.q64[c];
        __syncthreads();
    }
    const int lane = lane_id();
    // (the wave's number as a scalar: the id loads below are scalar loads then)
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t step = (int64_t)gridDim.x * (blockDim.x >> 6) * GATHER_ROWS;
    int32_t next[GATHER_ROWS];   // the ids of the next group: loaded one trip ahead, no id load in front of a trip's row loads
#pragma unroll
    for (int r = 0; r < GATHER_ROWS; ++r) next[r] = a.ids[min(wave * GATHER_ROWS + r, a.m - 1)];
    for (int64_t g = wave * GATHER_ROWS; g < a.m; g += step) {
        int64_t row[GATHER_ROWS];
#pragma unroll
        for (int r = 0; r < GATHER_ROWS; ++r) row[r] = next[r];   // (a short last group reads its last row again)
#pragma unroll
        for (int r = 0; r < GATHER_ROWS; ++r) next[r] = a.ids[min(g + step + r, a.m - 1)];
        // norm and lambda of row `lane` of the group, in flight under the dot products (lanes 0 .. GATHER_ROWS - 1)
        double nrm = 0.0, lam = 0.0;
        if (lane < GATHER_ROWS) {
            const int64_t j = lane == 0 ? row[0] : lane == 1 ? row[1] : lane == 2 ? row[2] : row[3];
            nrm = a.n64[j];
            lam = a.lam64[j];
        }
        double acc[GATHER_ROWS];
        gather_trip<F64, QLDS>(a.x32, a.x64, a.d, a.dp, row, qs, [&](int64_t e) { return a.q64[e]; }, lane, acc);
#pragma unroll
        for (int r = 0; r < GATHER_ROWS; ++r) acc[r] = wave_sum(acc[r]);   // (__shfl_xor butterfly: every lane holds the sums)
        if (lane < GATHER_ROWS && g + lane < a.m) {
            const double dot = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
            const double den = sqrt(nrm * a.nq);
            const double c = den > 0.0 ? dot / den : 0.0;
            if constexpr (TAUS) {
#pragma unroll
                for (int j = 0; j < TAU_GROUP; ++j)   // (unrolled: taus[j] is a scalar load, j < nt a scalar compare)
                    if (j < args.nt) a.scores[j * args.ld + g + lane] = blend_score(args.taus[j], c, a.lq, lam);   // lanes 0 .. 3: 32 bytes a plane
            } else {
                a.scores[g + lane] = blend_score(a.tau, c, a.lq, lam);   // lanes 0 .. 3: one 32-byte store
            }
        }
    }
}

// ------------------------------------------------------------------ batched score kernel
// scores[q][i] for a tile of SB_ROWS gathered rows and SB_Q queries per block: an fp64 GEMM on v_mfma_f64_16x16x4_f64 with the
// operand layouts of gram_f64_kernel (as_feat.hip).  A operand = queries (lane l: query l & 15, k = l >> 4), B operand = gathered
// rows (lane l: position l & 15, k = l >> 4), so C/D has the position on its column (lane & 15) and the query on its row
// ((lane >> 4) + 4 reg): the 16 scores of one query a wave stores per register are 128 contiguous bytes.  Wave (wi, wj) owns 64
// positions x 32 queries: 4 x 2 accumulators.  K runs in stages of SB_K columns: the gathered rows (as stored: fp32 rows of
// [np][dp], 16 bytes per lane, 8 lanes a row; or the fp64 rows of [n][d], 8-byte aligned only: one double per lane, 32 lanes a
// row) and the query tile (fp64) go through LDS, the next stage's global loads are issued in front of a stage's MFMAs.  Row
// pitches against bank conflicts of the operand reads (the 16 positions x 2 k of a 32-lane group): fp64 tiles 34 doubles (68
// dwords, 64 banks: 32 distinct bank pairs), the fp32 tile 34 floats (32 banks for a 4-byte read: 32 distinct banks; its rows
// are 8-byte aligned, so a lane's 16 bytes are written as two 8-byte halves).  Tail rows, the zero queries that pad a tile and columns >= d are zeros in LDS:
// no branch inside the MFMA loop.  Every score is ONE accumulation chain over k = 0 .. dp - 1 in that order, whatever its
// position in a tile: identical rows score bit-equal for one query.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int SB_ROWS = 128;
constexpr int SB_Q = 64;          // the query tile: chunks are multiples of it
constexpr int SB_K = 32;
constexpr int SB_PQ = SB_K + 2;   // pitch of an fp64 tile row, doubles
constexpr int SB_PF = SB_K + 2;   // pitch of an fp32 tile row, floats

struct SubsetBatchArgs {
    const int32_t* ids;
    int64_t m;
    const float* x32;
    const double* x64;
    const double* n64;
    const double* lam64;
    const double* q64;   // [nqp][dp], nqp a multiple of SB_Q, rows >= nq zero
    const double* nq;    // [nqp] |q|^2
    const double* lq;    // [nqp] lambda_q
    double* scores;      // [nq][ld]
    int64_t ld, d, dp;
    int nq_valid;
    double tau;
};
struct SubsetBatchTausArgs {   // the tau sweep's (section 5.11)
    SubsetBatchArgs s;   // (s.tau is not read)
    int nt;
    double taus[TAU_GROUP];
};

// Args = SubsetBatchArgs: scores[q * ld + pos]; SubsetBatchTausArgs: the cosine is blended with each of nt <= TAU_GROUP taus into
// plane (q, j) of the chunk at scores[(q * nt + j) * ld + pos] -- a (query, tau) pair is a row of the selection kernels.  The two
// differ in the stores alone.
template <bool F64, class Args>
__global__ __launch_bounds__(256) void subset_score_batch_kernel(Args args) {
    constexpr bool TAUS = std::is_same<Args, SubsetBatchTausArgs>::value;
    const SubsetBatchArgs* base;
    if constexpr (TAUS) base = &args.s;
    else base = &args;
    const SubsetBatchArgs& a = *base;
    constexpr int PX = F64 ? SB_PQ : SB_PF;
    constexpr int NR = F64 ? 16 : 4;   // rows a thread stages per K stage
    __shared__ __attribute__((aligned(16))) double qs[SB_Q * SB_PQ];
    __shared__ __attribute__((aligned(16))) char xs_raw[SB_ROWS * PX * (F64 ? 8 : 4)];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
    const int lk = lane >> 4, lc = lane & 15;
    const int64_t row0 = (int64_t)blockIdx.x * SB_ROWS;
    const int64_t q0 = (int64_t)blockIdx.y * SB_Q;
    // staging maps.  fp32 rows: thread t holds floats 4 (t & 7) .. + 3 of rows (t >> 3) + 32 i; fp64 rows: double t & 31 of rows
    // (t >> 5) + 8 i; queries: doubles 2 (t & 15), + 1 of queries (t >> 4) + 16 i
    const int xc = F64 ? (tid & 31) : (tid & 7) * 4, xr = F64 ? (tid >> 5) : (tid >> 3), xstep = F64 ? 8 : 32;
    const int qc = (tid & 15) * 2, qr = tid >> 4;
    int64_t rbase[NR];   // element offset of the staged rows; -1: past the end of the list (zeros)
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int64_t pos = row0 + xr + xstep * i;
        rbase[i] = pos < a.m ? (int64_t)a.ids[pos] * (F64 ? a.d : a.dp) : -1;
    }
    const double* qsrc = a.q64 + (q0 + qr) * a.dp + qc;
    f32x4 vf[F64 ? 1 : NR];
    double vd[F64 ? NR : 1];
    f64x2 vq[4];
    auto load_stage = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (F64) vd[i] = (rbase[i] >= 0 && k0 + xc < a.d) ? a.x64[rbase[i] + k0 + xc] : 0.0;
            else vf[i] = rbase[i] >= 0 ? *(const f32x4*)(a.x32 + rbase[i] + k0 + xc) : f32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) vq[i] = *(const f64x2*)(qsrc + (int64_t)16 * i * a.dp + k0);
    };
    f64x4 acc[2][4];
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) acc[ib][jb] = f64x4{0.0, 0.0, 0.0, 0.0};
    load_stage(0);
    for (int64_t k0 = 0; k0 < a.dp; k0 += SB_K) {
        __syncthreads();   // the previous stage has been consumed
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (F64) ((double*)xs_raw)[(xr + xstep * i) * PX + xc] = vd[i];
            else {
                f32x2* dst = (f32x2*)((float*)xs_raw + (xr + xstep * i) * PX + xc);
                dst[0] = f32x2{vf[i][0], vf[i][1]};
                dst[1] = f32x2{vf[i][2], vf[i][3]};
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) *(f64x2*)(qs + (qr + 16 * i) * SB_PQ + qc) = vq[i];
        __syncthreads();
        if (k0 + SB_K < a.dp) load_stage(k0 + SB_K);   // in flight under the MFMAs below
#pragma unroll
        for (int ks = 0; ks < SB_K / 4; ++ks) {
            double av[2], bv[4];
#pragma unroll
            for (int ib = 0; ib < 2; ++ib) av[ib] = qs[(32 * wj + 16 * ib + lc) * SB_PQ + 4 * ks + lk];
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) {
                const int e = (64 * wi + 16 * jb + lc) * PX + 4 * ks + lk;
                bv[jb] = F64 ? ((const double*)xs_raw)[e] : (double)((const float*)xs_raw)[e];
            }
#pragma unroll
            for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                for (int jb = 0; jb < 4; ++jb) acc[ib][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ib], bv[jb], acc[ib][jb], 0, 0, 0);
        }
    }
    // C/D of v_mfma_f64_16x16x4_f64: col = lane & 15 (position), row = (lane >> 4) + 4 reg (query)
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
        const int64_t pos = row0 + 64 * wi + 16 * jb + lc;
        if (pos >= a.m) continue;
        const int64_t j = a.ids[pos];
        const double nrm = a.n64[j], lam = a.lam64[j];
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t q = q0 + 32 * wj + 16 * ib + lk + 4 * r;
                if (q < a.nq_valid) {
                    const double den = sqrt(nrm * a.nq[q]);
                    const double c = den > 0.0 ? acc[ib][jb][r] / den : 0.0;
                    if constexpr (TAUS) {
                        const double lq = a.lq[q];
                        double* dst = a.scores + q * args.nt * a.ld + pos;   // plane (q, j): 16 lanes store 128 contiguous bytes
#pragma unroll
                        for (int u = 0; u < TAU_GROUP; ++u)
                            if (u < args.nt) dst[u * a.ld] = blend_score(args.taus[u], c, lq, lam);
                    } else {
                        a.scores[q * a.ld + pos] = blend_score(a.tau, c, a.lq[q], lam);
                    }
                }
            }
    }
}

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

__device__ __forceinline__ void sel_hist_body(const double* __restrict__ scores, int64_t m, int k, int p, SubsetSel* state, unsigned int* hist) {
    __shared__ unsigned int lh[SEL_BINS];
    for (int b = threadIdx.x; b < SEL_BINS; b += blockDim.x) lh[b] = 0u;
    const SubsetSel st = sel_state(p, k, state, hist);   // (its barriers order the zeroing above, too)
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long hi = sel_ord(scores[i]);
        const unsigned int lo = ~(unsigned int)i;
        if (sel_match(hi, lo, st.t_hi, st.t_lo, p)) atomicAdd(&lh[sel_digit(hi, lo, p)], 1u);
    }
    __syncthreads();
    unsigned int* gh = hist + (int64_t)p * SEL_BINS;
    for (int b = threadIdx.x; b < SEL_BINS; b += blockDim.x)
        if (lh[b]) atomicAdd(&gh[b], lh[b]);
}
// The selection's kernels work on row blockIdx.y (subset_select_rows): the single query, a query of a batched chunk or a (query,
// tau) pair of a sweep, with its scores at stride ld and its own histograms, state, positions and result
__global__ __launch_bounds__(256) void subset_hist_batch_kernel(const double* __restrict__ scores, int64_t ld, int64_t m, int k, int p,
                                                                SubsetSel* state, unsigned int* hist) {
    const int64_t q = blockIdx.y;
    sel_hist_body(scores + q * ld, m, k, p, state + q * (SEL_PASSES + 1), hist + q * SEL_HIST_WORDS);
}

// the positions whose key is at or above T, in any order: exactly k of them
__device__ __forceinline__ void sel_collect_body(const double* __restrict__ scores, int64_t m, int k, SubsetSel* state, unsigned int* hist,
                                                 int32_t* sel_pos) {
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
__global__ __launch_bounds__(256) void subset_collect_batch_kernel(const double* __restrict__ scores, int64_t ld, int64_t m, int k,
                                                                   SubsetSel* state, unsigned int* hist, int32_t* sel_pos) {
    const int64_t q = blockIdx.y;
    sel_collect_body(scores + q * ld, m, k, state + q * (SEL_PASSES + 1), hist + q * SEL_HIST_WORDS, sel_pos + q * SUBSET_TOPK);
}

// One block: the selected entries (sel_pos; null: all m <= SUBSET_TOPK positions) ranked by (score descending, position
// ascending) -- positions of a sorted id list are in id order --, the first k published to the pinned result.
__device__ __forceinline__ void sel_sort_body(const double* __restrict__ scores, const int32_t* __restrict__ ids, int64_t m, int k,
                                              const int32_t* __restrict__ sel_pos, const unsigned int* __restrict__ sel_cnt, SubsetOut* out) {
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
__global__ __launch_bounds__(1024) void subset_sort_batch_kernel(const double* __restrict__ scores, int64_t ld, const int32_t* __restrict__ ids,
                                                                 int64_t m, int k, const int32_t* __restrict__ sel_pos,
                                                                 const unsigned int* __restrict__ hist, SubsetOut* out) {
    const int64_t q = blockIdx.y;
    sel_sort_body(scores + q * ld, ids, m, k, sel_pos ? sel_pos + q * SUBSET_TOPK : nullptr,
                  sel_pos ? hist + q * SEL_HIST_WORDS + (int64_t)SEL_PASSES * SEL_BINS : nullptr, out + q);
}

// ------------------------------------------------------------------ host side
// Room for a call in the work's one buffer set: query_rows rows of the query stage, score_doubles scores (never fewer than the
// handle's ids: the single-query forms write there) and the selection's scratch for sel_rows rows -- the pinned results
// (want_out) and the radix select's histograms, state and positions (want_hist).  Exact sizes; a buffer that is large enough
// stays as it is.  A buffer whose allocation failed is empty: the call fails, the next one asks again.
static as_status subset_reserve(SubsetWork* w, int64_t query_rows, int64_t score_doubles, int64_t sel_rows, bool want_out, bool want_hist) {
    AS_TRY(reserve_or_err(w->qd, query_rows * (w->dp + 2), "subset query stage"));
    AS_TRY(reserve_or_err(w->qh, query_rows * (w->dp + 2), "subset pinned query stage"));
    AS_TRY(reserve_or_err(w->scores, std::max(score_doubles, w->cap), "subset scores"));
    if (want_out) AS_TRY(reserve_or_err(w->out, sel_rows, "subset pinned results"));
    if (want_hist) {
        AS_TRY(reserve_or_err(w->hist, sel_rows * SEL_HIST_WORDS, "subset selection histograms"));
        AS_TRY(reserve_or_err(w->state, sel_rows * (SEL_PASSES + 1), "subset selection states"));
        AS_TRY(reserve_or_err(w->sel_pos, sel_rows * SUBSET_TOPK, "subset selected positions"));
    }
    return AS_OK;
}

void subset_work_free(SubsetWork* w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    range_work_free(w->range);
    fused_work_free(w->fused);
    grouped_work_free(w->grouped);
    maxsim_work_free(w->maxsim);
    for (int i = 0; i < 2; ++i)
        if (w->ev[i]) (void)hipEventDestroy(w->ev[i]);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;   // (the buffers free themselves)
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
    as_status s = AS_OK;
    if ((e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking)) != hipSuccess || (e = hipEventCreate(&w->ev[0])) != hipSuccess ||
        (e = hipEventCreate(&w->ev[1])) != hipSuccess) {
        set_err("subset: creation of the stream and events failed: %s", hipGetErrorString(e));
        s = e == hipErrorOutOfMemory ? AS_ENOMEM : AS_EHIP;
    }
    // what a single query needs: nothing is allocated per single query afterwards
    if (s == AS_OK) s = reserve_or_err(w->ids, w->cap, "subset ids");
    if (s == AS_OK) s = subset_reserve(w, 1, w->cap, 1, true, true);
    if (s != AS_OK) {
        subset_work_free(w);
        return s;
    }
    *out = w;
    return AS_OK;
}

as_status subset_set_ids(SubsetWork* w, const int32_t* ids_host, int64_t m) {
    if (m <= 0) return AS_OK;
    AS_HIP(hipMemcpyAsync(w->ids, ids_host, sizeof(int32_t) * m, hipMemcpyHostToDevice, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    return AS_OK;
}

// the single query as row 0 of the query stage, uploaded (its dp doubles: the kernels take |q|^2 and lambda_q by value)
static as_status subset_upload_query(const as_space* sp, SubsetWork* w, const double* query, double lambda_q) {
    stage_queries(w->qh, query, 0, 1, 1, sp->d, w->dp, &lambda_q);
    AS_HIP(hipMemcpyAsync(w->qd, w->qh, sizeof(double) * w->dp, hipMemcpyHostToDevice, w->stream));
    return AS_OK;
}

// scores[i] = S11 score of item ids[i], i < m, queued on the work's stream (the query is uploaded in front of the kernel)
as_status subset_score(const as_space* sp, SubsetWork* w, int64_t m, const double* query, double tau, double lambda_q) {
    if (m <= 0) return AS_OK;
    AS_TRY(subset_reserve(w, 1, w->cap, 1, true, true));   // (nothing to do unless a larger call's allocation failed)
    AS_TRY(subset_upload_query(sp, w, query, lambda_q));
    SubsetArgs a;
    a.ids = w->ids; a.m = m; a.x32 = sp->x32; a.x64 = sp->x64; a.n64 = sp->n64; a.lam64 = sp->lam64; a.q64 = w->qd;
    a.scores = w->scores; a.d = sp->d; a.dp = sp->dp; a.nq = w->qh[w->dp]; a.lq = lambda_q; a.tau = tau;
    const int64_t groups = (m + GATHER_ROWS - 1) / GATHER_ROWS;   // one per wave and trip
    const unsigned grid = (unsigned)filtered_grid(std::max<int64_t>(1, std::min<int64_t>((groups + 3) / 4, (int64_t)w->cus * SUB_BLOCKS_PER_CU)));
    const bool qlds = sp->dp <= GATHER_Q_LDS;
    const size_t lds = qlds ? sizeof(double) * (size_t)sp->dp : 0;
    if (w->timing) AS_HIP(hipEventRecord(w->ev[0], w->stream));
    if (sp->x64) {
        if (qlds) hipLaunchKernelGGL((subset_score_kernel<true, true, SubsetArgs>), dim3(grid), dim3(256), lds, w->stream, a);
        else hipLaunchKernelGGL((subset_score_kernel<true, false, SubsetArgs>), dim3(grid), dim3(256), 0, w->stream, a);
    } else {
        if (qlds) hipLaunchKernelGGL((subset_score_kernel<false, true, SubsetArgs>), dim3(grid), dim3(256), lds, w->stream, a);
        else hipLaunchKernelGGL((subset_score_kernel<false, false, SubsetArgs>), dim3(grid), dim3(256), 0, w->stream, a);
    }
    AS_HIP(hipGetLastError());
    if (w->timing) AS_HIP(hipEventRecord(w->ev[1], w->stream));
    return AS_OK;
}

// waits for the stream; under timing the score kernel's time is added to kernel_us (fresh: replaces it -- the single-query forms)
static as_status subset_wait(SubsetWork* w, bool fresh = false) {
    if (fresh && w->timing) w->kernel_us = 0.0;
    return sync_add_elapsed(w->stream, w->timing != 0, w->ev, &w->kernel_us);
}

// The first k of each of `rows` rows of m scores ([rows][ld]) by (score descending, position ascending) -> w->out[row], queued on
// the work's stream.  m <= SUBSET_TOPK: the sort alone; else one memset, the radix passes, collect and sort.
// ids: the position -> id table of the answer ([m] on the device): the work's ids, or a caller's own.
static as_status subset_select_rows(SubsetWork* w, const double* scores, const int32_t* ids, int64_t ld, int64_t m, int64_t k, int64_t rows) {
    const unsigned ny = (unsigned)rows;
    SubsetOut* out = w->out;
    if (m <= SUBSET_TOPK) {
        hipLaunchKernelGGL(subset_sort_batch_kernel, dim3(1, ny), dim3(1024), 0, w->stream, scores, ld, ids, m, (int)k, (const int32_t*)nullptr,
                           (const unsigned int*)nullptr, out);
    } else {
        unsigned int* hist = w->hist;
        SubsetSel* state = w->state;
        int32_t* sel_pos = w->sel_pos;
        AS_HIP(hipMemsetAsync(hist, 0, sizeof(unsigned int) * SEL_HIST_WORDS * (size_t)rows, w->stream));
        const unsigned gx = (unsigned)filtered_grid(std::min<int64_t>((m + 2047) / 2048, 512));
        for (int p = 0; p < SEL_PASSES; ++p)
            hipLaunchKernelGGL(subset_hist_batch_kernel, dim3(gx, ny), dim3(256), 0, w->stream, scores, ld, m, (int)k, p, state, hist);
        hipLaunchKernelGGL(subset_collect_batch_kernel, dim3(gx, ny), dim3(256), 0, w->stream, scores, ld, m, (int)k, state, hist, sel_pos);
        hipLaunchKernelGGL(subset_sort_batch_kernel, dim3(1, ny), dim3(1024), 0, w->stream, scores, ld, ids, m, (int)k, (const int32_t*)sel_pos,
                           (const unsigned int*)hist, out);
    }
    AS_HIP(hipGetLastError());
    return AS_OK;
}

// a row's pinned result, k entries, to the caller's arrays
as_status subset_list_out(const SubsetOut* o, int64_t k, int64_t* out_idx, double* out_score, int64_t* out_len) {
    if (o->len != k) {
        set_err("subset: the selection returned %lld of %lld entries", (long long)o->len, (long long)k);
        return AS_EHIP;
    }
    for (int64_t r = 0; r < k; ++r) {
        out_idx[r] = o->idx[r];
        out_score[r] = o->score[r];
    }
    *out_len = k;
    return AS_OK;
}

// the first k of the m scores by (score descending, position ascending) -> ids and scores; waits for the stream
as_status subset_select(SubsetWork* w, int64_t m, int64_t k, int64_t* out_idx, double* out_score, int64_t* out_len) {
    *out_len = 0;
    if (m <= 0 || k <= 0) return AS_OK;
    k = std::min<int64_t>(std::min<int64_t>(k, m), SUBSET_TOPK);
    AS_TRY(subset_select_rows(w, w->scores, w->ids, m, m, k, 1));
    AS_TRY(subset_wait(w, true));
    return subset_list_out(w->out, k, out_idx, out_score, out_len);
}

as_status subset_select_from(SubsetWork* w, const double* scores, int64_t m, int64_t k, int64_t* out_idx, double* out_score, int64_t* out_len) {
    return subset_select_from_table(w, scores, w->ids, m, k, out_idx, out_score, out_len);
}

as_status subset_select_from_table(SubsetWork* w, const double* scores, const int32_t* pos_ids, int64_t m, int64_t k, int64_t* out_idx,
                                   double* out_score, int64_t* out_len) {
    *out_len = 0;
    if (m <= 0 || k <= 0) return AS_OK;
    k = std::min<int64_t>(std::min<int64_t>(k, m), SUBSET_TOPK);
    AS_TRY(subset_reserve(w, 1, w->cap, 1, true, true));   // (nothing to do unless a larger call's allocation failed)
    AS_TRY(subset_select_rows(w, scores, pos_ids, m, m, k, 1));
    AS_HIP(hipStreamSynchronize(w->stream));
    return subset_list_out(w->out, k, out_idx, out_score, out_len);
}

as_status subset_select_rows_from(SubsetWork* w, const double* scores, const int32_t* pos_ids, int64_t ld, int64_t m, int64_t k, int64_t rows) {
    if (m <= 0 || k <= 0 || rows <= 0) return AS_OK;
    k = std::min<int64_t>(std::min<int64_t>(k, m), SUBSET_TOPK);
    AS_TRY(reserve_or_err(w->out, rows, "subset pinned results"));
    if (m > SUBSET_TOPK) {
        AS_TRY(reserve_or_err(w->hist, rows * SEL_HIST_WORDS, "subset selection histograms"));
        AS_TRY(reserve_or_err(w->state, rows * (SEL_PASSES + 1), "subset selection states"));
        AS_TRY(reserve_or_err(w->sel_pos, rows * SUBSET_TOPK, "subset selected positions"));
    }
    AS_TRY(subset_select_rows(w, scores, pos_ids, ld, m, k, rows));
    AS_HIP(hipStreamSynchronize(w->stream));
    return AS_OK;
}

// the m scores themselves, in the order of the ids; waits for the stream
as_status subset_scores_out(SubsetWork* w, int64_t m, double* out) {
    if (m <= 0) {
        AS_HIP(hipStreamSynchronize(w->stream));
        return AS_OK;
    }
    AS_HIP(hipMemcpyAsync(out, w->scores, sizeof(double) * m, hipMemcpyDeviceToHost, w->stream));
    return subset_wait(w, true);
}

// ------------------------------------------------------------------ batched forms
// Queries per chunk: the largest multiple of the score kernel's query tile whose scores ([chunk][m] doubles) fit this budget, at
// least one tile, at most SB_QC_MAX (the selection keeps 128 KiB of histograms and a 16 KiB pinned result per query); a sink
// that keeps device memory per query of its own (SubsetChunkSink::row_bytes) has it counted beside the scores.  Results never
// depend on it.
static std::atomic<int> g_subset_batch_mib{256};
void set_subset_batch_mib(int v) { g_subset_batch_mib.store(v > 0 ? v : 256, std::memory_order_relaxed); }

as_status subset_batch_run(const as_space* sp, SubsetWork* w, int64_t m, const double* queries, int64_t b, const double* lq,
                           const int32_t* status, double tau, int64_t k, int64_t stride, int64_t* out_idx, double* out_score,
                           int64_t* out_len, double* out_scores, const SubsetChunkSink* sink) {
    if (m <= 0 || b <= 0) return AS_OK;
    const bool sel = k > 0;
    if (sel) k = std::min<int64_t>(std::min<int64_t>(k, m), SUBSET_TOPK);
    const int64_t budget = (int64_t)g_subset_batch_mib.load(std::memory_order_relaxed) << 20;
    int64_t qc = budget / (m * (int64_t)sizeof(double) + (sink ? sink->row_bytes : 0)) / SB_Q * SB_Q;
    qc = std::min<int64_t>(std::max<int64_t>(qc, SB_Q), SB_QC_MAX);
    qc = std::min<int64_t>(qc, (b + SB_Q - 1) / SB_Q * SB_Q);
    AS_TRY(subset_reserve(w, qc, qc * m, qc, sel, sel && m > SUBSET_TOPK));
    const int64_t d = sp->d, dp = w->dp;
    w->kernel_us = 0.0;
    for (int64_t i0 = 0; i0 < b; i0 += qc) {
        const int64_t nb = std::min<int64_t>(qc, b - i0), nbp = (nb + SB_Q - 1) / SB_Q * SB_Q;
        stage_queries(w->qh, queries, i0, nb, nbp, d, dp, lq);
        AS_HIP(hipMemcpyAsync(w->qd, w->qh, sizeof(double) * (size_t)(nbp * (dp + 2)), hipMemcpyHostToDevice, w->stream));
        SubsetBatchArgs a;
        a.ids = w->ids; a.m = m; a.x32 = sp->x32; a.x64 = sp->x64; a.n64 = sp->n64; a.lam64 = sp->lam64; a.q64 = w->qd;
        a.nq = w->qd + nbp * dp; a.lq = a.nq + nbp; a.scores = w->scores; a.ld = m; a.d = d; a.dp = dp; a.nq_valid = (int)nb; a.tau = tau;
        const dim3 grid((unsigned)((m + SB_ROWS - 1) / SB_ROWS), (unsigned)(nbp / SB_Q));
        if (w->timing) AS_HIP(hipEventRecord(w->ev[0], w->stream));
        if (sp->x64) hipLaunchKernelGGL((subset_score_batch_kernel<true, SubsetBatchArgs>), grid, dim3(256), 0, w->stream, a);
        else hipLaunchKernelGGL((subset_score_batch_kernel<false, SubsetBatchArgs>), grid, dim3(256), 0, w->stream, a);
        AS_HIP(hipGetLastError());
        if (w->timing) AS_HIP(hipEventRecord(w->ev[1], w->stream));
        if (sel) {
            AS_TRY(subset_select_rows(w, w->scores, w->ids, m, m, k, nb));
        } else if (sink) {
            AS_TRY(sink->fn(sink->ctx, w, i0, nb, w->scores, m));   // (range search's waits for the stream: the wait below finds it idle)
        } else {
            // one copy per run of served queries: a zero-lambda query's row stays unwritten
            AS_TRY(for_served_runs(status, i0, nb, [&](int64_t t, int64_t u) -> as_status {
                AS_HIP(hipMemcpyAsync(out_scores + (i0 + t) * m, w->scores + t * m, sizeof(double) * (size_t)((u - t) * m), hipMemcpyDeviceToHost,
                                      w->stream));
                return AS_OK;
            }));
        }
        AS_TRY(subset_wait(w));
        if (sel)
            for (int64_t t = 0; t < nb; ++t) {
                const int64_t i = i0 + t;
                out_len[i] = 0;
                if (status[i] == AS_EZEROLAMBDA) continue;
                AS_TRY(subset_list_out(w->out + t, k, out_idx + i * stride, out_score + i * stride, out_len + i));
            }
    }
    return AS_OK;
}

// ------------------------------------------------------------------ tau sweeps
// A (query, tau) pair takes the place of a query of the batched forms: a row of the scores and of the selection.
as_status subset_sweep_run(const as_space* sp, SubsetWork* w, int64_t m, const double* query, double lambda_q, const double* taus, int64_t nt,
                           const int64_t* row, int64_t k, int64_t* out_idx, double* out_score, int64_t* out_len, double* out_scores,
                           int64_t* counts) {
    if (m <= 0 || nt <= 0) return AS_OK;
    const bool sel = k > 0;
    if (sel) k = std::min<int64_t>(std::min<int64_t>(k, m), SUBSET_TOPK);
    const int64_t gmax = std::min<int64_t>(nt, TAU_GROUP);
    AS_TRY(subset_reserve(w, 1, gmax * m, gmax, sel, sel && m > SUBSET_TOPK));
    AS_TRY(subset_upload_query(sp, w, query, lambda_q));
    SubsetTausArgs a;
    a.s.ids = w->ids; a.s.m = m; a.s.x32 = sp->x32; a.s.x64 = sp->x64; a.s.n64 = sp->n64; a.s.lam64 = sp->lam64; a.s.q64 = w->qd;
    a.s.scores = w->scores; a.s.d = sp->d; a.s.dp = sp->dp; a.s.nq = w->qh[w->dp]; a.s.lq = lambda_q; a.s.tau = 0.0;
    a.ld = m;
    const int64_t groups = (m + GATHER_ROWS - 1) / GATHER_ROWS;   // (the grid of subset_score)
    const unsigned grid = (unsigned)filtered_grid(std::max<int64_t>(1, std::min<int64_t>((groups + 3) / 4, (int64_t)w->cus * SUB_BLOCKS_PER_CU)));
    const bool qlds = sp->dp <= GATHER_Q_LDS;
    const size_t lds = qlds ? sizeof(double) * (size_t)sp->dp : 0;
    w->kernel_us = 0.0;
    for (int64_t g0 = 0; g0 < nt; g0 += TAU_GROUP) {
        const int64_t ng = std::min<int64_t>(TAU_GROUP, nt - g0);
        a.nt = (int)ng;
        for (int64_t j = 0; j < TAU_GROUP; ++j) a.taus[j] = j < ng ? taus[g0 + j] : 0.0;
        if (w->timing) AS_HIP(hipEventRecord(w->ev[0], w->stream));
        if (sp->x64) {
            if (qlds) hipLaunchKernelGGL((subset_score_kernel<true, true, SubsetTausArgs>), dim3(grid), dim3(256), lds, w->stream, a);
            else hipLaunchKernelGGL((subset_score_kernel<true, false, SubsetTausArgs>), dim3(grid), dim3(256), 0, w->stream, a);
        } else {
            if (qlds) hipLaunchKernelGGL((subset_score_kernel<false, true, SubsetTausArgs>), dim3(grid), dim3(256), lds, w->stream, a);
            else hipLaunchKernelGGL((subset_score_kernel<false, false, SubsetTausArgs>), dim3(grid), dim3(256), 0, w->stream, a);
        }
        AS_HIP(hipGetLastError());
        if (w->timing) AS_HIP(hipEventRecord(w->ev[1], w->stream));
        counts[0] += 1;
        counts[1] += ng;
        if (sel) AS_TRY(subset_select_rows(w, w->scores, w->ids, m, m, k, ng));
        else
            for (int64_t j = 0; j < ng; ++j)
                AS_HIP(hipMemcpyAsync(out_scores + row[g0 + j] * m, w->scores + j * m, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, w->stream));
        AS_TRY(subset_wait(w));
        if (sel)
            for (int64_t j = 0; j < ng; ++j) {
                const int64_t r = row[g0 + j];
                AS_TRY(subset_list_out(w->out + j, k, out_idx + r * k, out_score + r * k, out_len + r));
            }
    }
    return AS_OK;
}

as_status subset_batch_sweep_run(const as_space* sp, SubsetWork* w, int64_t m, const double* queries, int64_t b, const double* lq,
                                 const int32_t* status, const double* taus, int64_t nt, const int64_t* row, int64_t ntau, int64_t k,
                                 int64_t* out_idx, double* out_score, int64_t* out_len, double* out_scores, int64_t* counts) {
    if (m <= 0 || b <= 0 || nt <= 0) return AS_OK;
    const bool sel = k > 0;
    if (sel) k = std::min<int64_t>(std::min<int64_t>(k, m), SUBSET_TOPK);
    // taus per group: the planes of one query tile fit the budget; queries per chunk: subset_batch_run's rule over m * tg scores
    // a query, the pairs of a chunk at most SB_QC_MAX
    const int64_t budget = (int64_t)g_subset_batch_mib.load(std::memory_order_relaxed) << 20;
    int64_t tg = budget / (SB_Q * m * (int64_t)sizeof(double));
    tg = std::min<int64_t>(std::min<int64_t>(std::max<int64_t>(tg, 1), TAU_GROUP), nt);
    int64_t qc = budget / (m * tg * (int64_t)sizeof(double)) / SB_Q * SB_Q;
    qc = std::min<int64_t>(std::max<int64_t>(qc, SB_Q), SB_QC_MAX / tg / SB_Q * SB_Q);
    qc = std::min<int64_t>(qc, (b + SB_Q - 1) / SB_Q * SB_Q);
    AS_TRY(subset_reserve(w, qc, qc * tg * m, qc * tg, sel, sel && m > SUBSET_TOPK));
    const int64_t d = sp->d, dp = w->dp;
    w->kernel_us = 0.0;
    for (int64_t i0 = 0; i0 < b; i0 += qc) {
        const int64_t nb = std::min<int64_t>(qc, b - i0), nbp = (nb + SB_Q - 1) / SB_Q * SB_Q;
        stage_queries(w->qh, queries, i0, nb, nbp, d, dp, lq);
        AS_HIP(hipMemcpyAsync(w->qd, w->qh, sizeof(double) * (size_t)(nbp * (dp + 2)), hipMemcpyHostToDevice, w->stream));
        SubsetBatchTausArgs a;
        a.s.ids = w->ids; a.s.m = m; a.s.x32 = sp->x32; a.s.x64 = sp->x64; a.s.n64 = sp->n64; a.s.lam64 = sp->lam64; a.s.q64 = w->qd;
        a.s.nq = w->qd + nbp * dp; a.s.lq = a.s.nq + nbp; a.s.scores = w->scores; a.s.ld = m; a.s.d = d; a.s.dp = dp;
        a.s.nq_valid = (int)nb; a.s.tau = 0.0;
        const dim3 grid((unsigned)((m + SB_ROWS - 1) / SB_ROWS), (unsigned)(nbp / SB_Q));
        for (int64_t g0 = 0; g0 < nt; g0 += tg) {
            const int64_t ng = std::min<int64_t>(tg, nt - g0);
            a.nt = (int)ng;
            for (int64_t j = 0; j < TAU_GROUP; ++j) a.taus[j] = j < ng ? taus[g0 + j] : 0.0;
            if (w->timing) AS_HIP(hipEventRecord(w->ev[0], w->stream));
            if (sp->x64) hipLaunchKernelGGL((subset_score_batch_kernel<true, SubsetBatchTausArgs>), grid, dim3(256), 0, w->stream, a);
            else hipLaunchKernelGGL((subset_score_batch_kernel<false, SubsetBatchTausArgs>), grid, dim3(256), 0, w->stream, a);
            AS_HIP(hipGetLastError());
            if (w->timing) AS_HIP(hipEventRecord(w->ev[1], w->stream));
            counts[0] += 1;
            counts[1] += ng;
            if (sel) AS_TRY(subset_select_rows(w, w->scores, w->ids, m, m, k, nb * ng));
            else {
                // plane j of every query of a run of served queries in one strided copy: a zero-lambda query's rows stay unwritten
                AS_TRY(for_served_runs(status, i0, nb, [&](int64_t t, int64_t u) -> as_status {
                    for (int64_t j = 0; j < ng; ++j)
                        AS_HIP(hipMemcpy2DAsync(out_scores + ((i0 + t) * ntau + row[g0 + j]) * m, sizeof(double) * (size_t)(ntau * m),
                                                w->scores + (t * ng + j) * m, sizeof(double) * (size_t)(ng * m), sizeof(double) * (size_t)m,
                                                (size_t)(u - t), hipMemcpyDeviceToHost, w->stream));
                    return AS_OK;
                }));
            }
            AS_TRY(subset_wait(w));
            if (sel)
                for (int64_t t = 0; t < nb; ++t) {
                    const int64_t i = i0 + t;
                    if (status[i] == AS_EZEROLAMBDA) continue;   // (its out_len entries are zero already)
                    for (int64_t j = 0; j < ng; ++j) {
                        const int64_t r = i * ntau + row[g0 + j];
                        AS_TRY(subset_list_out(w->out + t * ng + j, k, out_idx + r * k, out_score + r * k, out_len + r));
                    }
                }
        }
    }
    return AS_OK;
}

}  // namespace as
