// Bound-pruned Lloyd iterations (section 5.30).  The answer is the one of as_kmeans (as_kmeans.hip): the same labels,
// hence -- through the ordering and update launches of that file, reused as they are -- the same centroid bits.  What changes is
// which rows an iteration multiplies with the centroids.  Every row keeps lb, a lower bound on its distance (not squared) to every
// centroid but its own (Hamerly's second bound).  After an update,
//   SHIFT    p[j] = |c'_j - c_j| rounded upward, a wave per centroid (kmb_shift_kernel); one block then finds the largest and the
//            second-largest p, the arg of the largest and max_j |c'_j|^2 (kmb_top_kernel) and clears the active list's length;
//   FILTER   one pass over the stored rows (kmb_filter_kernel): 16 lanes read a row and its own centroid's row (by label), du = the
//            squared distance by direct differences; lb <- (lb - p1) rounded downward (p2 where the label is the arg of p1).  The
//            row is SKIPPED -- it keeps its label, dist <- du -- only where 0 < lb < inf and du + 4 E_i < lb^2 (1 - mg), with
//            E_i = (2 d + 8) 2^-53 (|x_i|^2 + max_j |c_j|^2) the bound on a key's error: then the keys km_assign_kernel would
//            compute put the label strictly first (section 5.30 derives it), so the tie rule never matters.  Every other row with
//            a label >= 0 joins the active list by ballot compaction (one atomic per 64 rows), in any order;
//   ASSIGN   kmb_assign_kernel: km_assign_kernel's GEMM-argmin -- the same 128 x 64 x 32 tile, the same operand layouts, the same
//            ascending order of the columns in every accumulator, hence the same bits of every dot, key and dist -- over the rows
//            of a device list whose length is a device word (a block whose tile lies past it leaves), gathered by id through LDS.
//            Besides the best (key, j) every lane keeps the smallest key among the OTHERS; the cross-lane and cross-wave combines
//            merge such pairs.  It writes label, dist, lb = sqrt(max(0, second - E_i)) rounded downward, and adds the changed
//            labels to the device word.
// Iteration 1 runs ASSIGN over all rows.  The host reads one pinned copy of the words per iteration (changed labels, active rows).
// Not built: the half distances between centroids, Elkan's or Yinyang's group bounds, bounds kept across calls.
// Entry points: as_api.hip (as_kmeans_bounded, as_kmeans_assign2, as_kmeans_bounded_counters, as_kmeans_bounded_kernel_us).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>
#include <vector>

#include "as_common.hpp"

namespace as {

namespace {

typedef float kb_f32x2 __attribute__((ext_vector_type(2)));
typedef float kb_f32x4 __attribute__((ext_vector_type(4)));
typedef double kb_f64x2 __attribute__((ext_vector_type(2)));
typedef double kb_f64x4 __attribute__((ext_vector_type(4)));

constexpr int KB_ROWS = 128;   // the tile of km_assign_kernel: rows of a block,
constexpr int KB_C = 64;       // centroids of a tile (kp is a multiple of it),
constexpr int KB_K = 32;       // columns of a K stage (dp is a multiple of it)
constexpr int KB_P = KB_K + 2;
constexpr int KB_NONE = 0x7fffffff;
constexpr int KB_TOP_THREADS = 256;
constexpr int KB_SUM_THREADS = 1024;
// the words of KmbWork::bw
constexpr int KB_P1 = 0, KB_P2 = 1, KB_ARG = 2, KB_CMAX = 3;
// the words of KmeansWork::stat_d the loop uses: [0] changed labels, [1] the inertia's bits, [2] empty clusters (as_kmeans.hip),
constexpr int KB_LEN = 3;      // [3] the length of the active list

__device__ __forceinline__ double kb_inf() { return __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ double kb_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool kb_better(double ka, int ja, double kb, int jb) { return ka < kb || (ka == kb && ja < jb); }

// (key, j, sec) <- the merge with another such triple over disjoint centroids: the better pair, and the smallest key among all the
// others, which is the loser's best or one of the two seconds.  A NaN never enters (it compares false).
__device__ __forceinline__ void kb_merge(double& key, int& j, double& sec, double ok, int oj, double os) {
    const bool w = kb_better(ok, oj, key, j);
    const double lose = w ? key : ok;
    if (os < sec) sec = os;
    if (lose < sec) sec = lose;
    if (w) {
        key = ok;
        j = oj;
    }
}

struct KmbAssignArgs {
    const float* x32;
    const double* x64;
    const double* n64;
    const double* cent;    // [kp][dp]
    const double* cn;      // [kp]
    const double* bw;      // [KB_CMAX]
    const int32_t* ids;    // the rows of the list; null: position i is row i
    const unsigned long long* len_word;   // the list's length on the device; null: len
    int32_t* labels;       // written at the ROW (by_pos: at the position in the list)
    double* dist;
    double* second;        // may be null
    double* lb;            // may be null
    unsigned long long* changed;
    int64_t len, n, d, dp;
    int kp, by_pos, prev;  // prev: a label counts as changed where it differs from the one `labels` held; else wherever it is >= 0
    double e_scale, mg;    // (2 d + 8) 2^-53; the directed margin
};

// (two blocks per CU, as km_assign_kernel: see the register counts in DESIGN.md section 5.30)
template <bool F64>
__global__ __launch_bounds__(256, 2) void kmb_assign_kernel(KmbAssignArgs a) {
    constexpr int NR = F64 ? 16 : 4;   // rows a thread stages per K stage
    __shared__ __attribute__((aligned(16))) double cs[KB_C * KB_P];
    __shared__ __attribute__((aligned(16))) char xs_raw[KB_ROWS * KB_P * (F64 ? 8 : 4)];
    __shared__ double s_key[KB_ROWS];
    __shared__ double s_sec[KB_ROWS];
    __shared__ int s_j[KB_ROWS];
    __shared__ int s_row[KB_ROWS];     // the tile's rows; -1 past the list's end
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
    const int lk = lane >> 4, lc = lane & 15;
    // staging maps and operand layouts: km_assign_kernel (as_kmeans.hip)
    const int xc = F64 ? (tid & 31) : (tid & 7) * 4, xr = F64 ? (tid >> 5) : (tid >> 3), xstep = F64 ? 8 : 32;
    const int qc = (tid & 15) * 2, qr = tid >> 4;
    const int64_t ld = F64 ? a.d : a.dp;
    const int64_t len = a.len_word ? (int64_t)a.len_word[0] : a.len;
    const int64_t tiles = (len + KB_ROWS - 1) / KB_ROWS;
    const int64_t stages = (int64_t)(a.kp / KB_C) * (a.dp / KB_K);
    const double cmax = a.bw[KB_CMAX];
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t pos0 = tile * KB_ROWS;
        __syncthreads();   // the previous tile's rows have been read
        if (tid < KB_ROWS) {
            const int64_t pos = pos0 + tid;
            int64_t r = -1;
            if (pos < len) r = a.ids ? (int64_t)a.ids[pos] : pos;
            s_row[tid] = (r >= 0 && r < a.n) ? (int)r : -1;
        }
        __syncthreads();
        kb_f32x4 vf[F64 ? 1 : NR];
        double vd[F64 ? NR : 1];
        kb_f64x2 vq[4];
        auto load_stage = [&](int c0, int64_t k0) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int64_t r = s_row[xr + xstep * i];
                if constexpr (F64) vd[i] = (r >= 0 && k0 + xc < a.d) ? a.x64[r * ld + k0 + xc] : 0.0;
                else vf[i] = r >= 0 ? *(const kb_f32x4*)(a.x32 + r * ld + k0 + xc) : kb_f32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) vq[i] = *(const kb_f64x2*)(a.cent + (int64_t)(c0 + qr + 16 * i) * a.dp + k0 + qc);
        };
        double bk[4], sk[4];
        int bj[4];
        kb_f64x4 acc[2][4];
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            bk[jb] = kb_inf();
            sk[jb] = kb_inf();
            bj[jb] = KB_NONE;
#pragma unroll
            for (int ib = 0; ib < 2; ++ib) acc[ib][jb] = kb_f64x4{0.0, 0.0, 0.0, 0.0};
        }
        int c0 = 0;
        int64_t k0 = 0;
        load_stage(0, 0);
        for (int64_t s = 0; s < stages; ++s) {
            __syncthreads();   // the previous stage has been consumed
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                if constexpr (F64) ((double*)xs_raw)[(xr + xstep * i) * KB_P + xc] = vd[i];
                else {
                    kb_f32x2* dst = (kb_f32x2*)((float*)xs_raw + (xr + xstep * i) * KB_P + xc);
                    dst[0] = kb_f32x2{vf[i][0], vf[i][1]};
                    dst[1] = kb_f32x2{vf[i][2], vf[i][3]};
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) *(kb_f64x2*)(cs + (qr + 16 * i) * KB_P + qc) = vq[i];
            __syncthreads();
            int nc0 = c0;
            int64_t nk0 = k0 + KB_K;
            if (nk0 >= a.dp) {   // the next stage opens the next centroid tile
                nk0 = 0;
                nc0 += KB_C;
            }
            if (s + 1 < stages) load_stage(nc0, nk0);   // in flight under the MFMAs below
#pragma unroll
            for (int ks = 0; ks < KB_K / 4; ++ks) {
                double av[2], bv[4];
#pragma unroll
                for (int ib = 0; ib < 2; ++ib) av[ib] = cs[(32 * wj + 16 * ib + lc) * KB_P + 4 * ks + lk];
#pragma unroll
                for (int jb = 0; jb < 4; ++jb) {
                    const int e = (64 * wi + 16 * jb + lc) * KB_P + 4 * ks + lk;
                    bv[jb] = F64 ? ((const double*)xs_raw)[e] : (double)((const float*)xs_raw)[e];
                }
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb) acc[ib][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ib], bv[jb], acc[ib][jb], 0, 0, 0);
            }
            if (nk0 == 0) {
                // the tile's dots are complete.  C/D: col = lane & 15 (the row of block jb), row = (lane >> 4) + 4 reg (the centroid)
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = c0 + 32 * wj + 16 * ib + lk + 4 * r;
                        const double cnj = a.cn[j];
#pragma unroll
                        for (int jb = 0; jb < 4; ++jb) {
                            const double key = cnj - 2.0 * acc[ib][jb][r];
                            const bool win = kb_better(key, j, bk[jb], bj[jb]);
                            const double lose = win ? bk[jb] : key;
                            if (lose < sk[jb]) sk[jb] = lose;
                            if (win) {
                                bk[jb] = key;
                                bj[jb] = j;
                            }
                        }
                    }
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb) acc[ib][jb] = kb_f64x4{0.0, 0.0, 0.0, 0.0};
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
                kb_merge(bk[jb], bj[jb], sk[jb], ok, oj, os);
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
            kb_merge(mk, mj, ms, s_key[64 * wi + lane], s_j[64 * wi + lane], s_sec[64 * wi + lane]);
            const int64_t row = s_row[64 * wi + lane];
            const int label = mj == KB_NONE ? -1 : mj;
            bool ch = false;
            if (row >= 0) {
                const int64_t o = a.by_pos ? pos0 + 64 * wi + lane : row;
                double dd = kb_nan(), s2 = kb_nan(), lbv = kb_nan();
                if (label >= 0) {
                    const double nn = a.n64[row];
                    dd = nn + mk;
                    dd = dd < 0.0 ? 0.0 : dd;
                    s2 = nn + ms;
                    s2 = s2 < 0.0 ? 0.0 : s2;
                    ch = a.prev ? a.labels[o] != label : true;
                    // every other centroid's TRUE squared distance is at least s2 - E_i
                    const double t = s2 - a.e_scale * (nn + cmax);
                    lbv = t > 0.0 ? sqrt(t) * (1.0 - a.mg) : 0.0;
                }
                a.labels[o] = label;
                a.dist[o] = dd;
                if (a.second) a.second[o] = s2;
                if (a.lb) a.lb[o] = lbv;
            }
            const int nch = __popcll(__ballot(ch));
            if (lane == 0 && nch) atomicAdd(a.changed, (unsigned long long)nch);
        }
    }
}

// p[j] = |c'_j - c_j| rounded upward, a wave per centroid: lane partials over strided columns, the butterfly, one square root.  The
// margin covers the roundings of the sum; 2^-500 the squares that underflow.  An overflow or a NaN becomes +inf: no row is skipped.
__global__ __launch_bounds__(256) void kmb_shift_kernel(const double* __restrict__ cold, const double* __restrict__ cnew, double* __restrict__ p,
                                                        int k, int kp, int64_t dp, double mg) {
    const int lane = lane_id(), j = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (j >= kp) return;
    double s = 0.0;
    for (int64_t c = lane; c < dp; c += 64) {
        const double v = cnew[(int64_t)j * dp + c] - cold[(int64_t)j * dp + c];
        s += v * v;
    }
    s = wave_sum(s);
    if (lane == 0) {
        double v = j < k ? sqrt(s) * (1.0 + mg) + 0x1p-500 : 0.0;
        if (!(v < kb_inf())) v = kb_inf();
        p[j] = v;
    }
}

// One block: bw <- the largest shift, the second-largest, the arg of the largest (ties: the smallest j), max_j cn[j]; the active
// list's length <- 0.  p null (iteration 1): the shifts are 0.
__global__ __launch_bounds__(KB_TOP_THREADS) void kmb_top_kernel(const double* __restrict__ p, const double* __restrict__ cn, int k, double* bw,
                                                                 unsigned long long* stat) {
    __shared__ double s1[KB_TOP_THREADS], s2[KB_TOP_THREADS], sc[KB_TOP_THREADS];
    __shared__ int sa[KB_TOP_THREADS];
    const int tid = threadIdx.x;
    double p1 = -1.0, p2 = -1.0, c = 0.0;
    int arg = KB_NONE;
    for (int j = tid; j < k; j += KB_TOP_THREADS) {
        const double v = p ? p[j] : 0.0;
        if (v > p1) {   // (ascending j: a tie keeps the smaller one)
            p2 = p1;
            p1 = v;
            arg = j;
        } else if (v > p2) p2 = v;
        const double n = cn[j];
        c = n > c ? n : c;
    }
    s1[tid] = p1; s2[tid] = p2; sa[tid] = arg; sc[tid] = c;
    __syncthreads();
    for (int o = KB_TOP_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const double o1 = s1[tid + o], o2 = s2[tid + o];
            const int oa = sa[tid + o];
            if (o1 > s1[tid] || (o1 == s1[tid] && oa < sa[tid])) {
                s2[tid] = s1[tid] > o2 ? s1[tid] : o2;
                s1[tid] = o1;
                sa[tid] = oa;
            } else if (o1 > s2[tid]) s2[tid] = o1;
            sc[tid] = sc[tid + o] > sc[tid] ? sc[tid + o] : sc[tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        bw[KB_P1] = s1[0] < 0.0 ? 0.0 : s1[0];
        bw[KB_P2] = s2[0] < 0.0 ? 0.0 : s2[0];   // (k == 1: there is no other centroid)
        bw[KB_ARG] = (double)sa[0];
        bw[KB_CMAX] = sc[0];
        stat[KB_LEN] = 0ull;
    }
}

struct KmbFilterArgs {
    const float* x32;
    const double* x64;
    const double* n64;
    const double* cent;    // [kp][dp] the centroids after the update
    const double* bw;
    const int32_t* labels;
    double* dist;
    double* lb;
    int32_t* list;
    unsigned long long* stat;
    int64_t n, d, dp;
    double e_scale, mg;
};

// A wave per 64 consecutive rows and trip: 16 trips of 4 rows, 16 lanes a row; then lane l owns row l of the 64.
template <bool F64>
__global__ __launch_bounds__(256) void kmb_filter_kernel(KmbFilterArgs a) {
    const int lane = lane_id(), g = lane >> 4, l = lane & 15;
    const double p1 = a.bw[KB_P1], p2 = a.bw[KB_P2], cmax = a.bw[KB_CMAX];
    const int arg = (int)a.bw[KB_ARG];
    const int64_t chunks = (a.n + 63) / 64;
    for (int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); chunk < chunks; chunk += (int64_t)gridDim.x * 4) {   // (wave-uniform)
        const int64_t myrow = chunk * 64 + lane;
        const int mylab = myrow < a.n ? a.labels[myrow] : -1;
        double mydu = 0.0;
#pragma unroll 4
        for (int t = 0; t < 16; ++t) {
            const int lab = __shfl(mylab, 4 * t + g, 64);
            const int64_t row = chunk * 64 + 4 * t + g;
            double s = 0.0;
            if (lab >= 0) {
                const double* c = a.cent + (int64_t)lab * a.dp;
                if constexpr (F64) {
                    const double* x = a.x64 + row * a.d;
                    for (int64_t col = l; col < a.d; col += 16) {
                        const double v = x[col] - c[col];
                        s += v * v;
                    }
                } else {
                    const float* x = a.x32 + row * a.dp;
                    for (int64_t col = 4 * l; col < a.d; col += 64) {   // (dp is a multiple of 32: the four floats lie inside the row)
                        const kb_f32x4 xv = *(const kb_f32x4*)(x + col);
                        const kb_f64x2 ca = *(const kb_f64x2*)(c + col), cb = *(const kb_f64x2*)(c + col + 2);
                        const double v0 = (double)xv[0] - ca[0], v1 = (double)xv[1] - ca[1], v2 = (double)xv[2] - cb[0], v3 = (double)xv[3] - cb[1];
                        s += v0 * v0;
                        if (col + 1 < a.d) s += v1 * v1;
                        if (col + 2 < a.d) s += v2 * v2;
                        if (col + 3 < a.d) s += v3 * v3;
                    }
                }
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);
            const double v = __shfl(s, (lane & 3) * 16, 64);
            if ((lane >> 2) == t) mydu = v;
        }
        bool active = false;
        if (mylab >= 0) {
            double b = a.lb[myrow] - (mylab == arg ? p2 : p1);
            b = b > 0.0 ? b * (1.0 - a.mg) : b;
            a.lb[myrow] = b;
            const double e = a.e_scale * (a.n64[myrow] + cmax);
            if (b > 0.0 && b < kb_inf() && mydu + 4.0 * e < b * b * (1.0 - a.mg)) a.dist[myrow] = mydu;
            else active = true;
        }
        const unsigned long long m = __ballot(active);
        if (m) {
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(a.stat + KB_LEN, (unsigned long long)__popcll(m));
            base = __shfl(base, 0, 64);
            if (active) a.list[base + __popcll(m & ((1ull << lane) - 1))] = (int32_t)myrow;
        }
    }
}

// inertia = the dist of the rows with a label >= 0: thread t adds rows t, t + 1024, .. in that order, then the halving tree
__global__ __launch_bounds__(KB_SUM_THREADS) void kmb_inertia_kernel(const double* __restrict__ dist, const int32_t* __restrict__ labels, int64_t n,
                                                                     unsigned long long* stat) {
    __shared__ double p[KB_SUM_THREADS];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += KB_SUM_THREADS)
        if (labels[i] >= 0) s += dist[i];
    p[threadIdx.x] = s;
    __syncthreads();
    for (int o = KB_SUM_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) p[threadIdx.x] += p[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) stat[1] = (unsigned long long)__double_as_longlong(p[0]);
}

// ------------------------------------------------------------------ host side
std::atomic<int> g_kmb_grid_cap{0};

unsigned kmb_grid(int64_t blocks) {
    const int64_t cap = g_kmb_grid_cap.load(std::memory_order_relaxed);
    blocks = std::max<int64_t>(blocks, 1);
    return (unsigned)(cap > 0 ? std::min(blocks, cap) : blocks);
}

// the directed margin on p and lb: 2^-40, and wider where the d roundings of a sum of squares need it
double kmb_margin(int64_t dp) { return std::max(0x1p-40, (double)(dp + 8) * 0x1p-50); }

// one timed part: launch() between two events on the work's stream, added to us[part] (timing waits for it)
template <typename F>
as_status kmb_timed(KmeansWork* w, int part, F&& launch) {
    const bool on = kmeans_timing_on();
    if (on) AS_HIP(hipEventRecord(w->ev.e[0], w->stream));
    launch();
    AS_HIP(hipGetLastError());
    if (!on) return AS_OK;
    AS_HIP(hipEventRecord(w->ev.e[1], w->stream));
    AS_HIP(hipEventSynchronize(w->ev.e[1]));
    float ms = 0.0f;
    AS_HIP(hipEventElapsedTime(&ms, w->ev.e[0], w->ev.e[1]));
    w->bounded.us[part] += (double)ms * 1e3;
    return AS_OK;
}

struct KmbShape {
    int64_t n, d, dp;
    int k, kp;
    double e_scale, mg;
    KmbShape(const as_space* sp, int64_t k_) : n(sp->n), d(sp->d), dp(sp->dp), k((int)k_), kp(kmeans_loop_kp(k_)) {
        e_scale = (double)(2 * d + 8) * 0x1p-53;
        mg = kmb_margin(dp);
    }
};

// cn and the words of cent[cur]; p: the shifts of the update behind it, null at iteration 1
as_status kmb_prepare(const as_space* sp, KmeansWork* w, const KmbShape& s, int cur, const double* p) {
    AS_TRY(kmeans_loop_norms(sp, w, s.k, cur));
    hipLaunchKernelGGL(kmb_top_kernel, dim3(1), dim3(KB_TOP_THREADS), 0, w->stream, p, (const double*)w->cn, s.k, (double*)w->bounded.bw,
                       (unsigned long long*)w->stat_d);
    AS_HIP(hipGetLastError());
    return AS_OK;
}

KmbAssignArgs kmb_assign_args(const as_space* sp, KmeansWork* w, const KmbShape& s, int cur) {
    KmbAssignArgs a{};
    a.x32 = sp->x32; a.x64 = sp->x64; a.n64 = sp->n64; a.cent = w->cent[cur]; a.cn = w->cn; a.bw = w->bounded.bw;
    a.changed = w->stat_d; a.n = s.n; a.d = s.d; a.dp = s.dp; a.kp = s.kp; a.e_scale = s.e_scale; a.mg = s.mg;
    return a;
}

void kmb_assign_launch(const as_space* sp, KmeansWork* w, const KmbAssignArgs& a, int64_t rows) {
    const unsigned grid = kmb_grid((rows + KB_ROWS - 1) / KB_ROWS);
    if (sp->x64) hipLaunchKernelGGL(kmb_assign_kernel<true>, dim3(grid), dim3(256), 0, w->stream, a);
    else hipLaunchKernelGGL(kmb_assign_kernel<false>, dim3(grid), dim3(256), 0, w->stream, a);
}

as_status kmb_lloyd_run(const as_space* sp, const KmeansCall& c, int64_t* out_active, int64_t* counts) {
    KmeansWork* w;
    AS_TRY(kmeans_loop_begin(sp, c.k, true, &w));
    const KmbShape s(sp, c.k);
    KmbWork& b = w->bounded;
    AS_TRY(reserve_or_err(b.lb, s.n, "kmeans_bounded lower bounds"));
    AS_TRY(reserve_or_err(b.list, s.n, "kmeans_bounded active list"));
    AS_TRY(reserve_or_err(b.p, s.kp, "kmeans_bounded shifts"));
    AS_TRY(reserve_or_err(b.bw, 4, "kmeans_bounded words"));
    for (double& v : b.us) v = 0.0;
    const unsigned long long* host = w->stat_h;
    AS_TRY(kmeans_loop_upload(sp, w, c.k, 0, c.init));
    int cur = 0;
    bool converged = false, ordered = false;
    int64_t t = 0;
    while (t < c.max_iters) {
        ++t;
        KmbAssignArgs a = kmb_assign_args(sp, w, s, cur);
        a.labels = w->labels[0]; a.dist = w->dist; a.lb = b.lb; a.len = s.n;
        if (t > 1) {
            AS_TRY(kmb_timed(w, 0, [&] {
                hipLaunchKernelGGL(kmb_shift_kernel, dim3((unsigned)((s.kp + 3) / 4)), dim3(256), 0, w->stream, (const double*)w->cent[cur ^ 1],
                                   (const double*)w->cent[cur], (double*)b.p, s.k, s.kp, s.dp, s.mg);
            }));
            AS_TRY(kmb_prepare(sp, w, s, cur, b.p));
            KmbFilterArgs f{};
            f.x32 = sp->x32; f.x64 = sp->x64; f.n64 = sp->n64; f.cent = w->cent[cur]; f.bw = b.bw; f.labels = w->labels[0]; f.dist = w->dist;
            f.lb = b.lb; f.list = b.list; f.stat = w->stat_d; f.n = s.n; f.d = s.d; f.dp = s.dp; f.e_scale = s.e_scale; f.mg = s.mg;
            const unsigned grid = kmb_grid(std::min<int64_t>((s.n + 255) / 256, (int64_t)w->cus * 32));
            AS_TRY(kmb_timed(w, 1, [&] {
                if (sp->x64) hipLaunchKernelGGL(kmb_filter_kernel<true>, dim3(grid), dim3(256), 0, w->stream, f);
                else hipLaunchKernelGGL(kmb_filter_kernel<false>, dim3(grid), dim3(256), 0, w->stream, f);
            }));
            counts[5] += 1;
            counts[6] += 1;
            a.ids = b.list; a.len_word = (const unsigned long long*)w->stat_d + KB_LEN; a.prev = 1;
        } else {
            AS_TRY(kmb_prepare(sp, w, s, cur, nullptr));
        }
        AS_TRY(kmb_timed(w, 2, [&] { kmb_assign_launch(sp, w, a, s.n); }));
        counts[1] += 1;
        AS_TRY(kmeans_loop_read(w, 4, counts));
        counts[0] += 1;
        const unsigned long long active = t > 1 ? host[KB_LEN] : (unsigned long long)s.n;
        if (host[0] > active || active > (unsigned long long)s.n) {
            set_err("kmeans_bounded: the device reported %llu changed labels of %llu active rows of %lld items", host[0], active, (long long)s.n);
            return AS_EHIP;
        }
        c.out_changed[t - 1] = (int64_t)host[0];
        out_active[t - 1] = (int64_t)active;
        counts[7] += (int64_t)active;
        if (host[0] == 0) {
            converged = true;
            break;
        }
        AS_TRY(kmeans_loop_order(sp, w, c.k, 0, true, counts));
        AS_TRY(kmeans_loop_update(sp, w, c.k, cur, counts));
        cur ^= 1;
        ordered = true;
    }
    // the counts of the labels returned: the last ordering's unless the loop ended on an assignment (as kmeans_lloyd)
    if (converged || !ordered) AS_TRY(kmeans_loop_order(sp, w, c.k, 0, false, counts));
    hipLaunchKernelGGL(kmb_inertia_kernel, dim3(1), dim3(KB_SUM_THREADS), 0, w->stream, (const double*)w->dist, (const int32_t*)w->labels[0], s.n,
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
    b.us[3] = (double)t;
    return AS_OK;
}

as_status kmb_assign2_run(const as_space* sp, const double* cent, int64_t k, const int32_t* ids, int64_t m, int32_t* out_labels, double* out_dist,
                          double* out_second, int64_t* counts) {
    KmeansWork* w;
    AS_TRY(kmeans_loop_begin(sp, k, false, &w));
    const KmbShape s(sp, k);
    KmbWork& b = w->bounded;
    AS_TRY(reserve_or_err(b.bw, 4, "kmeans_bounded words"));
    AS_TRY(reserve_or_err(b.olab, m, "kmeans_assign2 labels"));
    AS_TRY(reserve_or_err(b.odist, m, "kmeans_assign2 distances"));
    AS_TRY(reserve_or_err(b.osec, m, "kmeans_assign2 runner-up distances"));
    if (ids) {
        AS_TRY(reserve_or_err(b.ids, m, "kmeans_assign2 ids"));
        AS_HIP(hipMemcpyAsync((int32_t*)b.ids, ids, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, w->stream));
    }
    AS_TRY(kmeans_loop_upload(sp, w, k, 0, cent));   // (waits: the ids have crossed too)
    AS_TRY(kmb_prepare(sp, w, s, 0, nullptr));
    KmbAssignArgs a = kmb_assign_args(sp, w, s, 0);
    a.ids = ids ? (const int32_t*)b.ids : nullptr; a.len = m; a.by_pos = 1;
    a.labels = b.olab; a.dist = b.odist; a.second = b.osec;
    kmb_assign_launch(sp, w, a, m);
    AS_HIP(hipGetLastError());
    counts[1] += 1;
    AS_HIP(hipMemcpyAsync(out_labels, (const int32_t*)b.olab, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipMemcpyAsync(out_dist, (const double*)b.odist, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipMemcpyAsync(out_second, (const double*)b.osec, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[4] += 1;
    return AS_OK;
}

// (a failed run leaves nothing on the stream when the caller releases the lock)
template <typename F>
as_status kmb_guard(const as_space* sp, F&& run) {
    const as_status s = run();
    if (s != AS_OK && sp->kmeans_ws && sp->kmeans_ws->stream) (void)hipStreamSynchronize(sp->kmeans_ws->stream);
    return s;
}

}  // namespace

void set_kmeans_bounded_grid_cap(int v) { g_kmb_grid_cap.store(v > 0 ? v : 0, std::memory_order_relaxed); }
// for the bounded spherical loop (as_kmeans_spherical_bounded.hip): a grid under the same cap, the same directed margin
unsigned kmeans_bounded_grid(int64_t blocks) { return kmb_grid(blocks); }
double kmeans_bounded_margin(int64_t dp) { return kmb_margin(dp); }
double kmeans_bounded_kernel_us(const KmeansWork* w, int part) { return w && part >= 0 && part < 4 ? w->bounded.us[part] : 0.0; }

as_status kmeans_bounded(const as_space* sp, const KmeansCall& c, int64_t* out_active, int64_t* counts) {
    return kmb_guard(sp, [&] { return kmb_lloyd_run(sp, c, out_active, counts); });
}
as_status kmeans_assign2(const as_space* sp, const double* cent, int64_t k, const int32_t* ids, int64_t m, int32_t* out_labels, double* out_dist,
                         double* out_second, int64_t* counts) {
    return kmb_guard(sp, [&] { return kmb_assign2_run(sp, cent, k, ids, m, out_labels, out_dist, out_second, counts); });
}

}  // namespace as
