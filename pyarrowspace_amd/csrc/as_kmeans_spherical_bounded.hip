// Bound-pruned spherical k-means (section 5.32).  The answer is the one of as_kmeans_spherical.hip: the same labels,
// hence -- through the ordering, update and unit launches of that loop, reused as they are -- the same centroid bits.  What changes
// is which rows an iteration multiplies with the centroids.  On unit vectors the chord |x^ - c~| = sqrt(2 - 2 cos) is a Euclidean
// metric and the largest cosine is the smallest chord, so Hamerly's single bound carries over: every live row keeps lb, a lower
// bound on its chord to every centroid but its own (c~: the stored centroid row, exactly normalised).  After an update,
//   SHIFT    p[j] = (|c'_j - c_j| + (d + 8) 2^-53) rounded upward, a wave per centroid (ksb_shift_kernel): the direct differences of
//            the two unit buffers the loop holds, plus the allowance for neither row being exactly unit; one block then finds the
//            largest and the second-largest p and the arg of the largest (ksb_top_kernel) and clears the active list's length;
//   FILTER   one pass over the stored rows (ksb_filter_kernel): 16 lanes read a row and its own centroid's row (by label) once and
//            form du2 = sum_c (fl(x_c w) - c'_c)^2 by direct differences and the own dot x . c'; lb <- (lb - p1) rounded downward
//            (p2 where the label is the arg of p1).  The row is SKIPPED -- it keeps its label, cos <- clamp(fl(dot w)) -- only
//            where lb > 0 and du2 + 9 E < lb^2 (1 - mg), E = (2 d + 16) 2^-53 the bound of S28 on a device cosine: then the dots
//            kms_assign_kernel would compute put the label strictly first (section 5.32 derives it), so the tie rule never
//            matters.  Every other row with a label >= 0 joins the active list by ballot compaction (one atomic per 64 rows);
//   ASSIGN   ksb_assign_kernel: kms_assign_kernel's GEMM-argmax -- the same 128 x 64 x 32 tile, the same operand layouts, the same
//            ascending order of the columns in every accumulator, hence the same bits of every dot and cos -- over the rows of a
//            device list whose length is a device word, gathered by id through LDS.  Besides the best (g, j) every lane keeps the
//            largest g among the OTHERS; the cross-lane and cross-wave combines merge such triples.  It writes label, cos,
//            lb = sqrt(max(0, 2 - 2 (second + E + 4 2^-53))) rounded downward, and adds the changed labels to the device word.
// Iteration 1 runs ASSIGN over all rows.  The host reads one pinned copy of the words per iteration (changed labels, active rows).
// The list, lb, p and the words are the bounded loop's buffers (KmbWork), in the roles they have there.
// Not built: a cosine-aware seeding, Hamerly's second test (the half chord to the nearest other centroid), bounds kept across calls.
// Entry points: as_api.hip (as_kmeans_spherical_bounded, as_kmeans_cos_assign2, as_kmeans_spherical_bounded_counters,
// as_kmeans_spherical_bounded_kernel_us).
#include <algorithm>
#include <cmath>
#include <limits>

#include "as_common.hpp"

// S28 rounds every product and every sum once, and the cos of a row must carry kms_assign_kernel's bits: no multiply of this file
// may be fused with the add behind it (as as_kmeans_spherical.hip)
#pragma clang fp contract(off)

namespace as {

namespace {

typedef float sb_f32x2 __attribute__((ext_vector_type(2)));
typedef float sb_f32x4 __attribute__((ext_vector_type(4)));
typedef double sb_f64x2 __attribute__((ext_vector_type(2)));
typedef double sb_f64x4 __attribute__((ext_vector_type(4)));

constexpr int SB_ROWS = 128;   // the tile of kms_assign_kernel: rows of a block,
constexpr int SB_C = 64;       // centroids of a tile (kp is a multiple of it),
constexpr int SB_K = 32;       // columns of a K stage (dp is a multiple of it)
constexpr int SB_P = SB_K + 2;
constexpr int SB_NONE = 0x7fffffff;
constexpr int SB_TOP_THREADS = 256;
constexpr int SB_SUM_THREADS = 1024;
// the words of KmbWork::bw
constexpr int SB_P1 = 0, SB_P2 = 1, SB_ARG = 2;
// the words of KmeansWork::stat_d the loop uses: [0] changed labels, [1] the cohesion's bits, [2] empty clusters (as_kmeans.hip),
constexpr int SB_LEN = 3;      // [3] the length of the active list

__device__ __forceinline__ double sb_inf() { return __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ double sb_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
// ks_better of as_kmeans_spherical.hip: the larger dot wins, ties go to the smaller j; a NaN compares false both ways
__device__ __forceinline__ bool sb_better(double ga, int ja, double gb, int jb) { return ga > gb || (ga == gb && ja < jb); }
__device__ __forceinline__ double sb_clamp(double c) {
    c = c < -1.0 ? -1.0 : c;
    return c > 1.0 ? 1.0 : c;
}

// (g, j, sec) <- the merge with another such triple over disjoint centroids: the better pair, and the largest dot among all the
// others, which is the loser's best or one of the two seconds.  A NaN never enters (it compares false).
__device__ __forceinline__ void sb_merge(double& g, int& j, double& sec, double og, int oj, double os) {
    const bool w = sb_better(og, oj, g, j);
    const double lose = w ? g : og;
    if (os > sec) sec = os;
    if (lose > sec) sec = lose;
    if (w) {
        g = og;
        j = oj;
    }
}

struct KsbAssignArgs {
    const float* x32;
    const double* x64;
    const double* w;       // [n] the row scales; NaN: a dead row
    const double* cent;    // [kp][dp] unit rows, the rows j >= k zero
    const int32_t* ids;    // the rows of the list; null: position i is row i
    const unsigned long long* len_word;   // the list's length on the device; null: len
    int32_t* labels;       // written at the ROW (by_pos: at the position in the list)
    double* cosv;
    double* second;        // may be null
    double* lb;            // may be null
    unsigned long long* changed;
    int64_t len, n, d, dp;
    int k, kp, by_pos, prev;   // prev: a label counts as changed where it differs from the one `labels` held; else wherever it is >= 0
    double e_lb, mg;           // (2 d + 20) 2^-53: S28's E and the rounding of the sum it joins; the directed margin
};

// (two blocks per CU, as kms_assign_kernel: see the register counts in DESIGN.md section 5.32)
template <bool F64>
__global__ __launch_bounds__(256, 2) void ksb_assign_kernel(KsbAssignArgs a) {
    constexpr int NR = F64 ? 16 : 4;   // rows a thread stages per K stage
    __shared__ __attribute__((aligned(16))) double cs[SB_C * SB_P];
    __shared__ __attribute__((aligned(16))) char xs_raw[SB_ROWS * SB_P * (F64 ? 8 : 4)];
    __shared__ double s_key[SB_ROWS];
    __shared__ double s_sec[SB_ROWS];
    __shared__ int s_j[SB_ROWS];
    __shared__ int s_row[SB_ROWS];     // the tile's rows; -1 past the list's end
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
    const int lk = lane >> 4, lc = lane & 15;
    // staging maps and operand layouts: km_assign_kernel (as_kmeans.hip)
    const int xc = F64 ? (tid & 31) : (tid & 7) * 4, xr = F64 ? (tid >> 5) : (tid >> 3), xstep = F64 ? 8 : 32;
    const int qc = (tid & 15) * 2, qr = tid >> 4;
    const int64_t ld = F64 ? a.d : a.dp;
    const int64_t len = a.len_word ? (int64_t)a.len_word[0] : a.len;
    const int64_t tiles = (len + SB_ROWS - 1) / SB_ROWS;
    const int64_t stages = (int64_t)(a.kp / SB_C) * (a.dp / SB_K);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t pos0 = tile * SB_ROWS;
        __syncthreads();   // the previous tile's rows have been read
        if (tid < SB_ROWS) {
            const int64_t pos = pos0 + tid;
            int64_t r = -1;
            if (pos < len) r = a.ids ? (int64_t)a.ids[pos] : pos;
            s_row[tid] = (r >= 0 && r < a.n) ? (int)r : -1;
        }
        __syncthreads();
        sb_f32x4 vf[F64 ? 1 : NR];
        double vd[F64 ? NR : 1];
        sb_f64x2 vq[4];
        auto load_stage = [&](int c0, int64_t k0) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int64_t r = s_row[xr + xstep * i];
                if constexpr (F64) vd[i] = (r >= 0 && k0 + xc < a.d) ? a.x64[r * ld + k0 + xc] : 0.0;
                else vf[i] = r >= 0 ? *(const sb_f32x4*)(a.x32 + r * ld + k0 + xc) : sb_f32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) vq[i] = *(const sb_f64x2*)(a.cent + (int64_t)(c0 + qr + 16 * i) * a.dp + k0 + qc);
        };
        double bk[4], sk[4];
        int bj[4];
        sb_f64x4 acc[2][4];
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            bk[jb] = -sb_inf();
            sk[jb] = -sb_inf();
            bj[jb] = SB_NONE;
#pragma unroll
            for (int ib = 0; ib < 2; ++ib) acc[ib][jb] = sb_f64x4{0.0, 0.0, 0.0, 0.0};
        }
        int c0 = 0;
        int64_t k0 = 0;
        load_stage(0, 0);
        for (int64_t s = 0; s < stages; ++s) {
            __syncthreads();   // the previous stage has been consumed
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                if constexpr (F64) ((double*)xs_raw)[(xr + xstep * i) * SB_P + xc] = vd[i];
                else {
                    sb_f32x2* dst = (sb_f32x2*)((float*)xs_raw + (xr + xstep * i) * SB_P + xc);
                    dst[0] = sb_f32x2{vf[i][0], vf[i][1]};
                    dst[1] = sb_f32x2{vf[i][2], vf[i][3]};
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) *(sb_f64x2*)(cs + (qr + 16 * i) * SB_P + qc) = vq[i];
            __syncthreads();
            int nc0 = c0;
            int64_t nk0 = k0 + SB_K;
            if (nk0 >= a.dp) {   // the next stage opens the next centroid tile
                nk0 = 0;
                nc0 += SB_C;
            }
            if (s + 1 < stages) load_stage(nc0, nk0);   // in flight under the MFMAs below
#pragma unroll
            for (int ks = 0; ks < SB_K / 4; ++ks) {
                double av[2], bv[4];
#pragma unroll
                for (int ib = 0; ib < 2; ++ib) av[ib] = cs[(32 * wj + 16 * ib + lc) * SB_P + 4 * ks + lk];
#pragma unroll
                for (int jb = 0; jb < 4; ++jb) {
                    const int e = (64 * wi + 16 * jb + lc) * SB_P + 4 * ks + lk;
                    bv[jb] = F64 ? ((const double*)xs_raw)[e] : (double)((const float*)xs_raw)[e];
                }
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb) acc[ib][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ib], bv[jb], acc[ib][jb], 0, 0, 0);
            }
            if (nk0 == 0) {
                // the tile's dots are complete.  C/D: col = lane & 15 (the row of block jb), row = (lane >> 4) + 4 reg (the centroid);
                // pad centroids leave by index
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = c0 + 32 * wj + 16 * ib + lk + 4 * r;
                        if (j < a.k) {
#pragma unroll
                            for (int jb = 0; jb < 4; ++jb) {
                                const double g = acc[ib][jb][r];
                                const bool win = sb_better(g, j, bk[jb], bj[jb]);
                                const double lose = win ? bk[jb] : g;
                                if (lose > sk[jb]) sk[jb] = lose;
                                if (win) {
                                    bk[jb] = g;
                                    bj[jb] = j;
                                }
                            }
                        }
                    }
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb) acc[ib][jb] = sb_f64x4{0.0, 0.0, 0.0, 0.0};
            }
            c0 = nc0;
            k0 = nk0;
        }
        // the four lane groups of a row (lanes lc, lc + 16, lc + 32, lc + 48)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const double ok = __shfl_xor(bk[jb], o, 64), os = __shfl_xor(sk[jb], o, 64);
                const int oj = __shfl_xor(bj[jb], o, 64);
                sb_merge(bk[jb], bj[jb], sk[jb], ok, oj, os);
            }
        // lane (lk, lc) takes row block lk: position 64 wi + lane of the tile
        double mk = lk == 0 ? bk[0] : lk == 1 ? bk[1] : lk == 2 ? bk[2] : bk[3];
        double ms = lk == 0 ? sk[0] : lk == 1 ? sk[1] : lk == 2 ? sk[2] : sk[3];
        int mj = lk == 0 ? bj[0] : lk == 1 ? bj[1] : lk == 2 ? bj[2] : bj[3];
        if (wj == 1) {
            s_key[64 * wi + lane] = mk;
            s_sec[64 * wi + lane] = ms;
            s_j[64 * wi + lane] = mj;
        }
        __syncthreads();
        if (wj == 0) {
            sb_merge(mk, mj, ms, s_key[64 * wi + lane], s_j[64 * wi + lane], s_sec[64 * wi + lane]);
            const int64_t row = s_row[64 * wi + lane];
            bool ch = false;
            if (row >= 0) {
                const int64_t o = a.by_pos ? pos0 + 64 * wi + lane : row;
                const double ws = a.w[row];
                int label = -1;
                double cv = sb_nan(), sv = sb_nan(), lbv = sb_nan();
                if (ws == ws && mj != SB_NONE) {
                    label = mj;
                    cv = sb_clamp(mk * ws);
                    sv = ms > -sb_inf() ? sb_clamp(ms * ws) : -sb_inf();   // (k == 1: there is no other centroid)
                    ch = a.prev ? a.labels[o] != label : true;
                    // every other centroid's TRUE cosine is at most sv + E, its chord at least sqrt(2 - 2 (sv + E))
                    const double t = 2.0 - 2.0 * (sv + a.e_lb);
                    lbv = t > 0.0 ? sqrt(t) * (1.0 - a.mg) : 0.0;
                }
                a.labels[o] = label;
                a.cosv[o] = cv;
                if (a.second) a.second[o] = sv;
                if (a.lb) a.lb[o] = lbv;
            }
            const int nch = __popcll(__ballot(ch));
            if (lane == 0 && nch) atomicAdd(a.changed, (unsigned long long)nch);
        }
    }
}

// p[j] = (|c'_j - c_j| + allow) rounded upward, a wave per centroid: lane partials over strided columns, the butterfly, one square
// root.  allow: the two rows' distances from their exactly normalised selves.  The margin covers the roundings of the sum; 2^-500
// the squares that underflow.  An overflow or a NaN becomes +inf: no row is skipped.
__global__ __launch_bounds__(256) void ksb_shift_kernel(const double* __restrict__ cold, const double* __restrict__ cnew, double* __restrict__ p,
                                                        int k, int kp, int64_t dp, double allow, double mg) {
    const int lane = lane_id(), j = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (j >= kp) return;
    double s = 0.0;
    for (int64_t c = lane; c < dp; c += 64) {
        const double v = cnew[(int64_t)j * dp + c] - cold[(int64_t)j * dp + c];
        s += v * v;
    }
    s = wave_sum(s);
    if (lane == 0) {
        double v = j < k ? (sqrt(s) + allow) * (1.0 + mg) + 0x1p-500 : 0.0;
        if (!(v < sb_inf())) v = sb_inf();
        p[j] = v;
    }
}

// One block: bw <- the largest shift, the second-largest, the arg of the largest (ties: the smallest j); the active list's length
// <- 0.
__global__ __launch_bounds__(SB_TOP_THREADS) void ksb_top_kernel(const double* __restrict__ p, int k, double* bw, unsigned long long* stat) {
    __shared__ double s1[SB_TOP_THREADS], s2[SB_TOP_THREADS];
    __shared__ int sa[SB_TOP_THREADS];
    const int tid = threadIdx.x;
    double p1 = -1.0, p2 = -1.0;
    int arg = SB_NONE;
    for (int j = tid; j < k; j += SB_TOP_THREADS) {
        const double v = p[j];
        if (v > p1) {   // (ascending j: a tie keeps the smaller one)
            p2 = p1;
            p1 = v;
            arg = j;
        } else if (v > p2) p2 = v;
    }
    s1[tid] = p1; s2[tid] = p2; sa[tid] = arg;
    __syncthreads();
    for (int o = SB_TOP_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const double o1 = s1[tid + o], o2 = s2[tid + o];
            const int oa = sa[tid + o];
            if (o1 > s1[tid] || (o1 == s1[tid] && oa < sa[tid])) {
                s2[tid] = s1[tid] > o2 ? s1[tid] : o2;
                s1[tid] = o1;
                sa[tid] = oa;
            } else if (o1 > s2[tid]) s2[tid] = o1;
        }
        __syncthreads();
    }
    if (tid == 0) {
        bw[SB_P1] = s1[0] < 0.0 ? 0.0 : s1[0];
        bw[SB_P2] = s2[0] < 0.0 ? 0.0 : s2[0];   // (k == 1: there is no other centroid)
        bw[SB_ARG] = (double)sa[0];
        stat[SB_LEN] = 0ull;
    }
}

struct KsbFilterArgs {
    const float* x32;
    const double* x64;
    const double* w;       // [n] the row scales
    const double* cent;    // [kp][dp] the unit centroids after the update
    const double* bw;
    const int32_t* labels;
    double* cosv;
    double* lb;
    int32_t* list;
    unsigned long long* stat;
    int64_t n, d, dp;
    double e_skip, mg;     // 9 E; the directed margin
};

// A wave per 64 consecutive rows and trip: 16 trips of 4 rows, 16 lanes a row (kmb_filter_kernel's mapping); then lane l owns row l
// of the 64.  One read of the row gives du2 (against fl(x w)) and the own dot (of x itself).
template <bool F64>
__global__ __launch_bounds__(256) void ksb_filter_kernel(KsbFilterArgs a) {
    const int lane = lane_id(), g = lane >> 4, l = lane & 15;
    const double p1 = a.bw[SB_P1], p2 = a.bw[SB_P2];
    const int arg = (int)a.bw[SB_ARG];
    const int64_t chunks = (a.n + 63) / 64;
    for (int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); chunk < chunks; chunk += (int64_t)gridDim.x * 4) {   // (wave-uniform)
        const int64_t myrow = chunk * 64 + lane;
        const int mylab = myrow < a.n ? a.labels[myrow] : -1;
        const double myw = mylab >= 0 ? a.w[myrow] : 0.0;
        double mydu = 0.0, mydot = 0.0;
#pragma unroll 4
        for (int t = 0; t < 16; ++t) {
            const int lab = __shfl(mylab, 4 * t + g, 64);
            const double ws = __shfl(myw, 4 * t + g, 64);
            const int64_t row = chunk * 64 + 4 * t + g;
            double s = 0.0, q = 0.0;
            if (lab >= 0) {
                const double* c = a.cent + (int64_t)lab * a.dp;
                if constexpr (F64) {
                    const double* x = a.x64 + row * a.d;
                    for (int64_t col = l; col < a.d; col += 16) {
                        const double xv = x[col], cv = c[col], v = xv * ws - cv;
                        s += v * v;
                        q += xv * cv;
                    }
                } else {
                    const float* x = a.x32 + row * a.dp;
                    for (int64_t col = 4 * l; col < a.d; col += 64) {   // (dp is a multiple of 32: the four floats lie inside the row)
                        const sb_f32x4 xv = *(const sb_f32x4*)(x + col);
                        const sb_f64x2 ca = *(const sb_f64x2*)(c + col), cb = *(const sb_f64x2*)(c + col + 2);
                        const double x0 = (double)xv[0], x1 = (double)xv[1], x2 = (double)xv[2], x3 = (double)xv[3];
                        const double v0 = x0 * ws - ca[0], v1 = x1 * ws - ca[1], v2 = x2 * ws - cb[0], v3 = x3 * ws - cb[1];
                        s += v0 * v0;
                        q += x0 * ca[0];
                        if (col + 1 < a.d) {
                            s += v1 * v1;
                            q += x1 * ca[1];
                        }
                        if (col + 2 < a.d) {
                            s += v2 * v2;
                            q += x2 * cb[0];
                        }
                        if (col + 3 < a.d) {
                            s += v3 * v3;
                            q += x3 * cb[1];
                        }
                    }
                }
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                s += __shfl_xor(s, o, 64);
                q += __shfl_xor(q, o, 64);
            }
            const double vs = __shfl(s, (lane & 3) * 16, 64), vq = __shfl(q, (lane & 3) * 16, 64);
            if ((lane >> 2) == t) {
                mydu = vs;
                mydot = vq;
            }
        }
        bool active = false;
        if (mylab >= 0) {
            double b = a.lb[myrow] - (mylab == arg ? p2 : p1);
            b = b > 0.0 ? b * (1.0 - a.mg) : b;
            a.lb[myrow] = b;
            if (b > 0.0 && mydu + a.e_skip < b * b * (1.0 - a.mg)) a.cosv[myrow] = sb_clamp(mydot * myw);
            else active = true;
        }
        const unsigned long long m = __ballot(active);
        if (m) {
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(a.stat + SB_LEN, (unsigned long long)__popcll(m));
            base = __shfl(base, 0, 64);
            if (active) a.list[base + __popcll(m & ((1ull << lane) - 1))] = (int32_t)myrow;
        }
    }
}

// cohesion = the cos of the rows with a label >= 0: thread t adds rows t, t + 1024, .. in that order, then the halving tree
__global__ __launch_bounds__(SB_SUM_THREADS) void ksb_cohesion_kernel(const double* __restrict__ cosv, const int32_t* __restrict__ labels, int64_t n,
                                                                      unsigned long long* stat) {
    __shared__ double p[SB_SUM_THREADS];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += SB_SUM_THREADS)
        if (labels[i] >= 0) s += cosv[i];
    p[threadIdx.x] = s;
    __syncthreads();
    for (int o = SB_SUM_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) p[threadIdx.x] += p[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) stat[1] = (unsigned long long)__double_as_longlong(p[0]);
}

// ------------------------------------------------------------------ host side
// one timed part: launch() between two events on the work's stream, added to us[part] (timing waits for it)
template <typename F>
as_status ksb_timed(KmeansWork* w, int part, F&& launch) {
    const bool on = kmeans_timing_on();
    if (on) AS_HIP(hipEventRecord(w->ev.e[0], w->stream));
    launch();
    AS_HIP(hipGetLastError());
    if (!on) return AS_OK;
    AS_HIP(hipEventRecord(w->ev.e[1], w->stream));
    AS_HIP(hipEventSynchronize(w->ev.e[1]));
    float ms = 0.0f;
    AS_HIP(hipEventElapsedTime(&ms, w->ev.e[0], w->ev.e[1]));
    w->sbounded.us[part] += (double)ms * 1e3;
    return AS_OK;
}

struct KsbShape {
    int64_t n, d, dp;
    int k, kp;
    double e, allow, mg;
    KsbShape(const as_space* sp, int64_t k_) : n(sp->n), d(sp->d), dp(sp->dp), k((int)k_), kp(kmeans_loop_kp(k_)) {
        e = (double)(2 * d + 16) * 0x1p-53;     // S28's E
        allow = (double)(d + 8) * 0x1p-53;      // twice (d / 2 + 4) 2^-53: how far a stored unit row lies from its normalised self
        mg = kmeans_bounded_margin(dp);
    }
};

KsbAssignArgs ksb_assign_args(const as_space* sp, KmeansWork* w, const KsbShape& s, int cur) {
    KsbAssignArgs a{};
    a.x32 = sp->x32; a.x64 = sp->x64; a.w = w->spherical.w; a.cent = w->cent[cur]; a.changed = w->stat_d;
    a.n = s.n; a.d = s.d; a.dp = s.dp; a.k = s.k; a.kp = s.kp; a.e_lb = s.e + 4.0 * 0x1p-53; a.mg = s.mg;
    return a;
}

void ksb_assign_launch(const as_space* sp, KmeansWork* w, const KsbAssignArgs& a, int64_t rows) {
    const unsigned grid = kmeans_bounded_grid((rows + SB_ROWS - 1) / SB_ROWS);
    if (sp->x64) hipLaunchKernelGGL(ksb_assign_kernel<true>, dim3(grid), dim3(256), 0, w->stream, a);
    else hipLaunchKernelGGL(ksb_assign_kernel<false>, dim3(grid), dim3(256), 0, w->stream, a);
}

// counts: [0 .. 6] as kmeans_spherical's, [7] filter launches, [8] shift launches, [9] the rows that went through the GEMM
as_status ksb_lloyd_run(const as_space* sp, const KmeansCall& c, int64_t* out_active, int64_t* counts) {
    KmeansWork* w;
    AS_TRY(kmeans_spherical_loop_begin(sp, c.k, true, &w, counts));
    const KsbShape s(sp, c.k);
    KmbWork& b = w->bounded;
    AS_TRY(reserve_or_err(b.lb, s.n, "kmeans_spherical_bounded lower bounds"));
    AS_TRY(reserve_or_err(b.list, s.n, "kmeans_spherical_bounded active list"));
    AS_TRY(reserve_or_err(b.p, s.kp, "kmeans_spherical_bounded shifts"));
    AS_TRY(reserve_or_err(b.bw, 4, "kmeans_spherical_bounded words"));
    for (double& v : w->sbounded.us) v = 0.0;
    const unsigned long long* host = w->stat_h;
    AS_TRY(kmeans_loop_upload(sp, w, c.k, 0, c.init));
    AS_TRY(kmeans_spherical_loop_unit(sp, w, c.k, 0, -1, false, counts));
    int cur = 0;
    bool converged = false, ordered = false;
    int64_t t = 0;
    while (t < c.max_iters) {
        ++t;
        KsbAssignArgs a = ksb_assign_args(sp, w, s, cur);
        a.labels = w->labels[0]; a.cosv = w->dist; a.lb = b.lb; a.len = s.n;
        if (t > 1) {
            AS_TRY(ksb_timed(w, 0, [&] {
                hipLaunchKernelGGL(ksb_shift_kernel, dim3((unsigned)((s.kp + 3) / 4)), dim3(256), 0, w->stream, (const double*)w->cent[cur ^ 1],
                                   (const double*)w->cent[cur], (double*)b.p, s.k, s.kp, s.dp, s.allow, s.mg);
                hipLaunchKernelGGL(ksb_top_kernel, dim3(1), dim3(SB_TOP_THREADS), 0, w->stream, (const double*)b.p, s.k, (double*)b.bw,
                                   (unsigned long long*)w->stat_d);
            }));
            KsbFilterArgs f{};
            f.x32 = sp->x32; f.x64 = sp->x64; f.w = w->spherical.w; f.cent = w->cent[cur]; f.bw = b.bw; f.labels = w->labels[0]; f.cosv = w->dist;
            f.lb = b.lb; f.list = b.list; f.stat = w->stat_d; f.n = s.n; f.d = s.d; f.dp = s.dp; f.e_skip = 9.0 * s.e; f.mg = s.mg;
            const unsigned grid = kmeans_bounded_grid(std::min<int64_t>((s.n + 255) / 256, (int64_t)w->cus * 32));
            AS_TRY(ksb_timed(w, 1, [&] {
                if (sp->x64) hipLaunchKernelGGL(ksb_filter_kernel<true>, dim3(grid), dim3(256), 0, w->stream, f);
                else hipLaunchKernelGGL(ksb_filter_kernel<false>, dim3(grid), dim3(256), 0, w->stream, f);
            }));
            counts[7] += 1;
            counts[8] += 1;
            a.ids = b.list; a.len_word = (const unsigned long long*)w->stat_d + SB_LEN; a.prev = 1;
        }
        AS_TRY(ksb_timed(w, 2, [&] { ksb_assign_launch(sp, w, a, s.n); }));
        counts[1] += 1;
        AS_TRY(kmeans_loop_read(w, t > 1 ? 4 : 1, counts));   // (changed labels and the list's length together)
        counts[0] += 1;
        const unsigned long long active = t > 1 ? host[SB_LEN] : (unsigned long long)s.n;
        if (host[0] > active || active > (unsigned long long)s.n) {
            set_err("kmeans_spherical_bounded: the device reported %llu changed labels of %llu active rows of %lld items", host[0], active,
                    (long long)s.n);
            return AS_EHIP;
        }
        c.out_changed[t - 1] = (int64_t)host[0];
        out_active[t - 1] = (int64_t)active;
        counts[9] += (int64_t)active;
        if (host[0] == 0) {
            converged = true;
            break;
        }
        AS_TRY(kmeans_loop_order(sp, w, c.k, 0, true, counts));
        AS_TRY(kmeans_spherical_loop_update(sp, w, c.k, cur, counts));   // (its unit launch clears the changed word for the next assignment)
        cur ^= 1;
        ordered = true;
    }
    // the counts of the labels returned: the last ordering's unless the loop ended on an assignment (as kmeans_lloyd)
    if (converged || !ordered) AS_TRY(kmeans_loop_order(sp, w, c.k, 0, false, counts));
    hipLaunchKernelGGL(ksb_cohesion_kernel, dim3(1), dim3(SB_SUM_THREADS), 0, w->stream, (const double*)w->dist, (const int32_t*)w->labels[0], s.n,
                       (unsigned long long*)w->stat_d);
    AS_HIP(hipGetLastError());
    AS_TRY(kmeans_loop_download(sp, w, c.k, cur, c.out_centroids));
    AS_HIP(hipMemcpyAsync(c.out_labels, (const int32_t*)w->labels[0], sizeof(int32_t) * (size_t)s.n, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipMemcpyAsync(c.out_counts32, (const int32_t*)w->counts, sizeof(int32_t) * (size_t)s.k, hipMemcpyDeviceToHost, w->stream));
    AS_TRY(kmeans_loop_read(w, 3, counts));
    c.info->iterations = t;
    c.info->converged = converged ? 1 : 0;
    c.info->empty = (int64_t)host[2];
    memcpy(&c.info->inertia, &host[1], sizeof(double));
    w->sbounded.us[3] = (double)t;
    return AS_OK;
}

as_status ksb_assign2_run(const as_space* sp, const double* cent, int64_t k, const int32_t* ids, int64_t m, int32_t* out_labels, double* out_cos,
                          double* out_second, int64_t* counts) {
    KmeansWork* w;
    AS_TRY(kmeans_spherical_loop_begin(sp, k, false, &w, counts));
    const KsbShape s(sp, k);
    KmbWork& b = w->bounded;
    AS_TRY(reserve_or_err(b.olab, m, "kmeans_cos_assign2 labels"));
    AS_TRY(reserve_or_err(b.odist, m, "kmeans_cos_assign2 cosines"));
    AS_TRY(reserve_or_err(b.osec, m, "kmeans_cos_assign2 runner-up cosines"));
    if (ids) {
        AS_TRY(reserve_or_err(b.ids, m, "kmeans_cos_assign2 ids"));
        AS_HIP(hipMemcpyAsync((int32_t*)b.ids, ids, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, w->stream));
    }
    AS_TRY(kmeans_loop_upload(sp, w, k, 0, cent));   // (waits: the ids have crossed too)
    AS_TRY(kmeans_spherical_loop_unit(sp, w, k, 0, -1, false, counts));
    KsbAssignArgs a = ksb_assign_args(sp, w, s, 0);
    a.ids = ids ? (const int32_t*)b.ids : nullptr; a.len = m; a.by_pos = 1;
    a.labels = b.olab; a.cosv = b.odist; a.second = b.osec;
    ksb_assign_launch(sp, w, a, m);
    AS_HIP(hipGetLastError());
    counts[1] += 1;
    AS_HIP(hipMemcpyAsync(out_labels, (const int32_t*)b.olab, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipMemcpyAsync(out_cos, (const double*)b.odist, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipMemcpyAsync(out_second, (const double*)b.osec, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[4] += 1;
    return AS_OK;
}

// (a failed run leaves nothing on the stream when the caller releases the lock)
template <typename F>
as_status ksb_guard(const as_space* sp, F&& run) {
    const as_status s = run();
    if (s != AS_OK && sp->kmeans_ws && sp->kmeans_ws->stream) (void)hipStreamSynchronize(sp->kmeans_ws->stream);
    return s;
}

}  // namespace

// parts: 0 shift launches (shift and top), 1 filter launches, 2 assign launches, 3 iterations
double kmeans_spherical_bounded_kernel_us(const KmeansWork* w, int part) { return w && part >= 0 && part < 4 ? w->sbounded.us[part] : 0.0; }

as_status kmeans_spherical_bounded(const as_space* sp, const KmeansCall& c, int64_t* out_active, int64_t* counts) {
    return ksb_guard(sp, [&] { return ksb_lloyd_run(sp, c, out_active, counts); });
}
as_status kmeans_cos_assign2(const as_space* sp, const double* cent, int64_t k, const int32_t* ids, int64_t m, int32_t* out_labels, double* out_cos,
                             double* out_second, int64_t* counts) {
    return ksb_guard(sp, [&] { return ksb_assign2_run(sp, cent, k, ids, m, out_labels, out_cos, out_second, counts); });
}

}  // namespace as
