// k-means over the items (section 5.28).  Items are the stored items (x64 where the space keeps it, else
// x32 widened: what as_get_item returns); centroids are k <= 4096 rows of d doubles, on the device [kp][dp], zero padded.
//   ASSIGN   key(i, j) = fl(cn[j] - fl(2 dot(i, j))), labels[i] = the j of the smallest key (ties: the smallest j; a NaN key never
//            wins; no comparable key: -1), dist[i] = max(0, fl(n64[i] + key)).  km_assign_kernel is an fp64 GEMM on
//            v_mfma_f64_16x16x4_f64 with the operand layouts of subset_score_batch_kernel (as_subset.hip) whose N x k products never
//            leave the accumulators: a block of 4 waves owns KM_ROWS consecutive rows (no id gather), the CENTROID tile of KM_C is
//            its outer loop, the K stages of KM_K columns the inner one; after a centroid tile's last stage every lane turns its
//            32 accumulators (4 row blocks x 8 centroids) into keys and folds them into four running (key, j) minima; after the last
//            tile the four lane groups of a row meet by cross-lane moves, the two waves that share rows through LDS, and the 64
//            lanes of one wave of each pair own one row each: label, dist, the count of changed labels (one integer atomic per
//            wave) and the inertia partial of the 64 rows (a fixed halving tree).  Pad centroids carry cn = NaN: their keys never
//            compare.  The grid strides over the row tiles ("kmeans_grid_cap"): a row's answer is a function of the row alone.
//   ORDER    a stable counting sort of the item ids by label: per-wave LDS histograms over units of consecutive rows -> table
//            [units][k]; one scan launch -> the exclusive prefixes along the units on top of the clusters' starts, the clusters'
//            segment starts, the number of empty clusters; one scatter launch places row r at base + (same label earlier in the
//            unit) + (same label in lower lanes, by ballot).  No atomic decides a position: members are ascending in id.
//   UPDATE   pinned in bits given the labels: P_s = the members [256 s, 256 s + 256) of a cluster added one by one in that order
//            from the first one's row (a wave per (cluster, segment, 64-column slab)); T = P_0 + P_1 + .. in that order; c' = T /
//            count; an empty cluster keeps its centroid (km_update_final_kernel).
// The Lloyd loop reads one pinned word per iteration (the changed labels).  Entry points: as_api.hip (as_kmeans_assign, as_kmeans,
// as_kmeans_update, as_kmeans_counters, as_kmeans_kernel_us).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>
#include <new>

#include "as_common.hpp"

namespace as {

namespace {

typedef float km_f32x2 __attribute__((ext_vector_type(2)));
typedef float km_f32x4 __attribute__((ext_vector_type(4)));
typedef double km_f64x2 __attribute__((ext_vector_type(2)));
typedef double km_f64x4 __attribute__((ext_vector_type(4)));

constexpr int KM_ROWS = 128;        // rows of a block's tile
constexpr int KM_C = 64;            // centroids of a tile: kp is a multiple of it
constexpr int KM_K = 32;            // columns of a K stage: dp is a multiple of it (COL_PAD)
constexpr int KM_P = KM_K + 2;      // pitch of a tile row in LDS, elements (the bank argument of as_subset.hip)
constexpr int KM_SEG = 256;         // members of an update segment: part of the definition (S25)
constexpr int KM_NONE = 0x7fffffff;
constexpr int KM_UNITS_MAX = 1024;  // units of the counting sort at most: the scan walks them one after the other
constexpr int KM_SORT_THREADS = 128;   // two waves, each with k LDS counters of its own (32 KiB at k = 4096)

struct KmAssignArgs {
    const float* x32;
    const double* x64;
    const double* n64;
    const double* cent;   // [kp][dp]
    const double* cn;     // [kp]
    int32_t* labels;      // [n]
    const int32_t* prev;  // [n] the labels before; null: every label >= 0 counts as changed
    double* dist;         // [n]
    double* ipart;        // [2 tiles] the inertia partials of 64 rows each
    unsigned long long* changed;
    int64_t n, d, dp;
    int kp;
};

__device__ __forceinline__ bool km_better(double ka, int ja, double kb, int jb) { return ka < kb || (ka == kb && ja < jb); }

// cn[j] = |c_j|^2, a wave per centroid: lane partials over strided columns, then the butterfly; NaN on the pad rows.  Clears the
// changed-labels word for the assign launch behind it.
__global__ __launch_bounds__(256) void km_norms_kernel(const double* __restrict__ cent, double* __restrict__ cn, unsigned long long* stat, int k,
                                                       int kp, int64_t dp) {
    if (blockIdx.x == 0 && threadIdx.x == 0) stat[0] = 0ull;
    const int lane = lane_id(), j = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (j >= kp) return;
    double s = 0.0;
    for (int64_t c = lane; c < dp; c += 64) {
        const double v = cent[(int64_t)j * dp + c];
        s += v * v;
    }
    s = wave_sum(s);
    if (lane == 0) cn[j] = j < k ? s : __longlong_as_double(0x7ff8000000000000LL);
}

// (two blocks per CU: without the bound the fp64-row instantiation takes 279 registers and one wave per SIMD)
template <bool F64>
__global__ __launch_bounds__(256, 2) void km_assign_kernel(KmAssignArgs a) {
    constexpr int NR = F64 ? 16 : 4;   // rows a thread stages per K stage
    __shared__ __attribute__((aligned(16))) double cs[KM_C * KM_P];
    __shared__ __attribute__((aligned(16))) char xs_raw[KM_ROWS * KM_P * (F64 ? 8 : 4)];
    __shared__ double s_key[KM_ROWS];
    __shared__ int s_j[KM_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
    const int lk = lane >> 4, lc = lane & 15;
    // staging maps (as_subset.hip).  fp32 rows: thread t holds floats 4 (t & 7) .. + 3 of rows (t >> 3) + 32 i; fp64 rows: double
    // t & 31 of rows (t >> 5) + 8 i; centroids: doubles 2 (t & 15), + 1 of centroids (t >> 4) + 16 i
    const int xc = F64 ? (tid & 31) : (tid & 7) * 4, xr = F64 ? (tid >> 5) : (tid >> 3), xstep = F64 ? 8 : 32;
    const int qc = (tid & 15) * 2, qr = tid >> 4;
    const int64_t ld = F64 ? a.d : a.dp;
    const int64_t tiles = (a.n + KM_ROWS - 1) / KM_ROWS;
    const int64_t stages = (int64_t)(a.kp / KM_C) * (a.dp / KM_K);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * KM_ROWS;
        km_f32x4 vf[F64 ? 1 : NR];
        double vd[F64 ? NR : 1];
        km_f64x2 vq[4];
        auto load_stage = [&](int c0, int64_t k0) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int64_t pos = row0 + xr + xstep * i;
                if constexpr (F64) vd[i] = (pos < a.n && k0 + xc < a.d) ? a.x64[pos * ld + k0 + xc] : 0.0;
                else vf[i] = pos < a.n ? *(const km_f32x4*)(a.x32 + pos * ld + k0 + xc) : km_f32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) vq[i] = *(const km_f64x2*)(a.cent + (int64_t)(c0 + qr + 16 * i) * a.dp + k0 + qc);
        };
        double bk[4];
        int bj[4];
        km_f64x4 acc[2][4];
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            bk[jb] = key_traits<double>::inf();
            bj[jb] = KM_NONE;
#pragma unroll
            for (int ib = 0; ib < 2; ++ib) acc[ib][jb] = km_f64x4{0.0, 0.0, 0.0, 0.0};
        }
        int c0 = 0;
        int64_t k0 = 0;
        load_stage(0, 0);
        for (int64_t s = 0; s < stages; ++s) {
            __syncthreads();   // the previous stage has been consumed
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                if constexpr (F64) ((double*)xs_raw)[(xr + xstep * i) * KM_P + xc] = vd[i];
                else {
                    km_f32x2* dst = (km_f32x2*)((float*)xs_raw + (xr + xstep * i) * KM_P + xc);
                    dst[0] = km_f32x2{vf[i][0], vf[i][1]};
                    dst[1] = km_f32x2{vf[i][2], vf[i][3]};
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) *(km_f64x2*)(cs + (qr + 16 * i) * KM_P + qc) = vq[i];
            __syncthreads();
            int nc0 = c0;
            int64_t nk0 = k0 + KM_K;
            if (nk0 >= a.dp) {   // the next stage opens the next centroid tile
                nk0 = 0;
                nc0 += KM_C;
            }
            if (s + 1 < stages) load_stage(nc0, nk0);   // in flight under the MFMAs below
#pragma unroll
            for (int ks = 0; ks < KM_K / 4; ++ks) {
                double av[2], bv[4];
#pragma unroll
                for (int ib = 0; ib < 2; ++ib) av[ib] = cs[(32 * wj + 16 * ib + lc) * KM_P + 4 * ks + lk];
#pragma unroll
                for (int jb = 0; jb < 4; ++jb) {
                    const int e = (64 * wi + 16 * jb + lc) * KM_P + 4 * ks + lk;
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
                            if (km_better(key, j, bk[jb], bj[jb])) {
                                bk[jb] = key;
                                bj[jb] = j;
                            }
                        }
                    }
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb) acc[ib][jb] = km_f64x4{0.0, 0.0, 0.0, 0.0};
            }
            c0 = nc0;
            k0 = nk0;
        }
        // the four lane groups of a row (lanes lc, lc + 16, lc + 32, lc + 48)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const double ok = __shfl_xor(bk[jb], o, 64);
                const int oj = __shfl_xor(bj[jb], o, 64);
                if (km_better(ok, oj, bk[jb], bj[jb])) {
                    bk[jb] = ok;
                    bj[jb] = oj;
                }
            }
        // lane (lk, lc) takes row block lk: row 64 wi + lane of the tile
        double mk = lk == 0 ? bk[0] : lk == 1 ? bk[1] : lk == 2 ? bk[2] : bk[3];
        int mj = lk == 0 ? bj[0] : lk == 1 ? bj[1] : lk == 2 ? bj[2] : bj[3];
        if (wj == 1) {
            s_key[64 * wi + lane] = mk;
            s_j[64 * wi + lane] = mj;
        }
        __syncthreads();
        if (wj == 0) {
            const double ok = s_key[64 * wi + lane];
            const int oj = s_j[64 * wi + lane];
            if (km_better(ok, oj, mk, mj)) {
                mk = ok;
                mj = oj;
            }
            const int64_t row = row0 + 64 * wi + lane;
            const bool live = row < a.n;
            const int label = mj == KM_NONE ? -1 : mj;
            double dd = __longlong_as_double(0x7ff8000000000000LL);
            bool ch = false;
            if (live) {
                if (label >= 0) {
                    dd = a.n64[row] + mk;
                    dd = dd < 0.0 ? 0.0 : dd;
                    ch = a.prev ? a.prev[row] != label : true;
                }
                a.labels[row] = label;
                a.dist[row] = dd;
            }
            const int nch = __popcll(__ballot(ch));
            if (lane == 0 && nch) atomicAdd(a.changed, (unsigned long long)nch);
            double v = live && label >= 0 ? dd : 0.0;   // the inertia partial of these 64 rows: a fixed halving tree
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) a.ipart[tile * 2 + wi] = v;
        }
    }
}

// inertia = the partials in a fixed order: thread t adds partials t, t + 256, .. in that order, then the halving tree
__global__ __launch_bounds__(256) void km_inertia_kernel(const double* __restrict__ ipart, int64_t m, unsigned long long* stat) {
    __shared__ double p[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 256) s += ipart[i];
    p[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) p[threadIdx.x] += p[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) stat[1] = (unsigned long long)__double_as_longlong(p[0]);
}

// ---- member ordering
__global__ __launch_bounds__(256) void km_clear_kernel(int32_t* counts, int kp) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j < kp) counts[j] = 0;
}

// table[u][j] = the rows of unit u with label j, counts[j] += the same.  A wave per unit and trip, its k counters in LDS.
__global__ __launch_bounds__(KM_SORT_THREADS) void km_hist_kernel(const int32_t* __restrict__ labels, int64_t n, int k, int64_t unit_rows,
                                                                  int64_t units, int32_t* __restrict__ table, int32_t* counts) {
    extern __shared__ int32_t km_cnt[];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    int32_t* cnt = km_cnt + wv * k;
    for (int64_t u = (int64_t)blockIdx.x * (KM_SORT_THREADS / 64) + wv; u < units; u += (int64_t)gridDim.x * (KM_SORT_THREADS / 64)) {
        for (int j = lane; j < k; j += 64) cnt[j] = 0;
        AS_LDS_FENCE();
        const int64_t r1 = min(n, (u + 1) * unit_rows);
        for (int64_t r = u * unit_rows + lane; r < r1; r += 64) {
            const int32_t l = labels[r];
            if (l >= 0) atomicAdd(&cnt[l], 1);
        }
        AS_LDS_FENCE();
        for (int j = lane; j < k; j += 64) {
            const int32_t c = cnt[j];
            table[u * k + j] = c;
            if (c) atomicAdd(&counts[j], c);
        }
        AS_LDS_FENCE();
    }
}

// A wave per 64 clusters: start[j] = the members of the clusters below j, segstart[j] = their segments (start[k], segstart[k]: the
// totals); table[u][j] <- start[j] + the rows of units below u with label j; block 0 counts the empty clusters.
__global__ __launch_bounds__(64) void km_scan_kernel(int32_t* table, const int32_t* __restrict__ counts, int32_t* start, int32_t* segstart,
                                                     unsigned long long* stat, int k, int64_t units) {
    const int lane = threadIdx.x, j0 = (int)blockIdx.x * 64, j = j0 + lane;
    int below = 0, sbelow = 0, empty = 0;
    for (int t = lane; t < j0; t += 64) {
        const int c = counts[t];
        below += c;
        sbelow += (c + KM_SEG - 1) / KM_SEG;
    }
    below = wave_sum(below);
    sbelow = wave_sum(sbelow);
    if (blockIdx.x == 0) {
        for (int t = lane; t < k; t += 64) empty += counts[t] == 0 ? 1 : 0;
        empty = wave_sum(empty);
        if (lane == 0) stat[2] = (unsigned long long)empty;
    }
    const int c = j < k ? counts[j] : 0, sg = (c + KM_SEG - 1) / KM_SEG;
    int incl = c, sincl = sg;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64), sv = __shfl_up(sincl, o, 64);
        if (lane >= o) {
            incl += v;
            sincl += sv;
        }
    }
    if (j >= k) return;
    const int first = below + incl - c;
    start[j] = first;
    segstart[j] = sbelow + sincl - sg;
    if (j == k - 1) {
        start[k] = first + c;
        segstart[k] = sbelow + sincl;
    }
    int run = first;
#pragma unroll 8
    for (int64_t u = 0; u < units; ++u) {
        const int t = table[u * k + j];
        table[u * k + j] = run;
        run += t;
    }
}

// members[base + (same label earlier in the unit) + (same label in lower lanes)] = row: a wave walks its unit 64 rows at a time, its
// k running positions in LDS.
__global__ __launch_bounds__(KM_SORT_THREADS) void km_scatter_kernel(const int32_t* __restrict__ labels, int64_t n, int k, int64_t unit_rows,
                                                                     int64_t units, const int32_t* __restrict__ table, int32_t* __restrict__ members) {
    extern __shared__ int32_t km_cnt[];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    int32_t* cnt = km_cnt + wv * k;
    for (int64_t u = (int64_t)blockIdx.x * (KM_SORT_THREADS / 64) + wv; u < units; u += (int64_t)gridDim.x * (KM_SORT_THREADS / 64)) {
        for (int j = lane; j < k; j += 64) cnt[j] = table[u * k + j];
        AS_LDS_FENCE();
        const int64_t r1 = min(n, (u + 1) * unit_rows);
        for (int64_t r = u * unit_rows; r < r1; r += 64) {   // (wave-uniform: every lane meets every ballot)
            const int64_t row = r + lane;
            const int32_t l = row < r1 ? labels[row] : -1;
            unsigned long long todo = __ballot(l >= 0);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const int32_t ll = __shfl(l, leader, 64);
                const unsigned long long same = __ballot(l == ll);
                if (l == ll) members[cnt[ll] + __popcll(same & ((1ull << lane) - 1))] = (int32_t)row;
                AS_LDS_FENCE();
                if (lane == leader) cnt[ll] += __popcll(same);
                AS_LDS_FENCE();
                todo &= ~same;
            }
        }
    }
}

// ---- update
struct KmUpdateArgs {
    const float* x32;
    const double* x64;
    const int32_t* members;
    const int32_t* counts;
    const int32_t* start;      // [k + 1]
    const int32_t* segstart;   // [k + 1]
    double* part;              // [segments][dp]
    const double* cent_old;    // [kp][dp]
    double* cent_new;
    int64_t d, dp;
    int k, kp;
};

// A wave per (segment slot, 64-column slab): the slot's cluster by bisection of segstart, its members' rows added in order.
template <bool F64>
__global__ __launch_bounds__(256) void km_update_part_kernel(KmUpdateArgs a) {
    const int lane = lane_id();
    const int slot = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (slot >= a.segstart[a.k]) return;
    int lo = 0, hi = a.k;   // segstart[lo] <= slot < segstart[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.segstart[mid] <= slot) lo = mid;
        else hi = mid;
    }
    const int seg = slot - a.segstart[lo];
    const int32_t* mem = a.members + a.start[lo] + KM_SEG * seg;
    const int m = min(KM_SEG, a.counts[lo] - KM_SEG * seg);
    const int64_t col = (int64_t)blockIdx.y * 64 + lane;
    if (col >= a.d) return;
    double acc = 0.0;
    for (int t = 0; t < m; t += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t id = mem[min(t + u, m - 1)];
            v[u] = F64 ? a.x64[id * a.d + col] : (double)a.x32[id * a.dp + col];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (t + u < m) acc = t + u == 0 ? v[u] : acc + v[u];
    }
    a.part[(int64_t)slot * a.dp + col] = acc;
}

// c_j' = (P_0 + P_1 + ..) / count, a thread per (cluster, column); an empty cluster, a pad row and a pad column keep what they held
__global__ __launch_bounds__(256) void km_update_final_kernel(KmUpdateArgs a) {
    const int j = blockIdx.y;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= a.dp) return;
    double out = a.cent_old[(int64_t)j * a.dp + col];
    if (j < a.k && col < a.d && a.counts[j] > 0) {
        const int s0 = a.segstart[j], ns = a.segstart[j + 1] - s0;
        double T = a.part[(int64_t)s0 * a.dp + col];
        for (int s = 1; s < ns; ++s) T = T + a.part[(int64_t)(s0 + s) * a.dp + col];
        out = T / (double)a.counts[j];
    }
    a.cent_new[(int64_t)j * a.dp + col] = out;
}

// ------------------------------------------------------------------ host side
std::atomic<int> g_kmeans_grid_cap{0};
std::atomic<int> g_kmeans_timing{0};

unsigned km_grid(int64_t blocks) {
    const int64_t cap = g_kmeans_grid_cap.load(std::memory_order_relaxed);
    blocks = std::max<int64_t>(blocks, 1);
    return (unsigned)(cap > 0 ? std::min(blocks, cap) : blocks);
}

// the shapes of a call: kp, the units of the counting sort, the update's segment slots at most
struct KmShape {
    int64_t n, d, dp;
    int k, kp;
    int64_t unit_rows, units, slots;
    KmShape(const as_space* sp, int64_t k_) : n(sp->n), d(sp->d), dp(sp->dp), k((int)k_) {
        kp = (k + KM_C - 1) / KM_C * KM_C;
        const int64_t waves = (n + 63) / 64;
        unit_rows = 64 * ((waves + KM_UNITS_MAX - 1) / KM_UNITS_MAX);
        units = (n + unit_rows - 1) / unit_rows;
        slots = n / KM_SEG + k + 1;   // sum_j ceil(count_j / 256) <= n / 256 + k
    }
};

// one timed part: the launches between begin() and end() on the work's stream, added to *us (timing waits for them)
struct KmTimer {
    KmeansWork* w;
    bool on;
    as_status begin() const {
        if (on) AS_HIP(hipEventRecord(w->ev.e[0], w->stream));
        return AS_OK;
    }
    as_status end(double* us) const {
        if (!on) return AS_OK;
        AS_HIP(hipEventRecord(w->ev.e[1], w->stream));
        AS_HIP(hipEventSynchronize(w->ev.e[1]));
        float ms = 0.0f;
        AS_HIP(hipEventElapsedTime(&ms, w->ev.e[0], w->ev.e[1]));
        *us += (double)ms * 1e3;
        return AS_OK;
    }
};

as_status km_work_get(const as_space* sp, KmeansWork** out) {
    if (!sp->kmeans_ws) {
        KmeansWork* w = new (std::nothrow) KmeansWork();
        if (!w) {
            set_err("kmeans: out of host memory");
            return AS_ENOMEM;
        }
        w->device = sp->device;
        if (hipDeviceGetAttribute(&w->cus, hipDeviceAttributeMultiprocessorCount, sp->device) != hipSuccess || w->cus <= 0) w->cus = 256;
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking)) != hipSuccess || (e = w->ev.create()) != hipSuccess) {
            set_err("kmeans: creation of the stream and events failed: %s", hipGetErrorString(e));
            kmeans_work_free(w);
            return AS_EHIP;
        }
        sp->kmeans_ws = w;
    }
    *out = sp->kmeans_ws;
    return AS_OK;
}

as_status km_reserve(KmeansWork* w, const KmShape& s, bool order) {
    for (int i = 0; i < 2; ++i) {
        AS_TRY(reserve_or_err(w->labels[i], s.n, "kmeans labels"));
        AS_TRY(reserve_or_err(w->cent[i], (int64_t)s.kp * s.dp, "kmeans centroids"));
    }
    AS_TRY(reserve_or_err(w->dist, s.n, "kmeans distances"));
    AS_TRY(reserve_or_err(w->cn, s.kp, "kmeans centroid norms"));
    AS_TRY(reserve_or_err(w->ipart, 2 * ((s.n + KM_ROWS - 1) / KM_ROWS), "kmeans inertia partials"));
    AS_TRY(reserve_or_err(w->stat_d, 4, "kmeans words"));
    AS_TRY(reserve_or_err(w->stat_h, 4, "kmeans pinned words"));
    if (order) {
        AS_TRY(reserve_or_err(w->members, s.n, "kmeans member list"));
        AS_TRY(reserve_or_err(w->table, s.units * s.k, "kmeans histogram table"));
        AS_TRY(reserve_or_err(w->counts, 3 * (int64_t)s.kp + 2, "kmeans cluster counts"));
        AS_TRY(reserve_or_err(w->part, s.slots * s.dp, "kmeans update partials"));
    }
    return AS_OK;
}

// the caller's [k][d] centroids into cent[which] ([kp][dp], zero padded); waits (the source is the caller's memory)
as_status km_upload(KmeansWork* w, const KmShape& s, int which, const double* host) {
    double* dst = w->cent[which];
    AS_HIP(hipMemsetAsync(dst, 0, sizeof(double) * (size_t)s.kp * (size_t)s.dp, w->stream));
    AS_HIP(hipMemcpy2DAsync(dst, sizeof(double) * (size_t)s.dp, host, sizeof(double) * (size_t)s.d, sizeof(double) * (size_t)s.d, (size_t)s.k,
                            hipMemcpyHostToDevice, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    return AS_OK;
}
as_status km_download(KmeansWork* w, const KmShape& s, int which, double* host) {
    AS_HIP(hipMemcpy2DAsync(host, sizeof(double) * (size_t)s.d, (const double*)w->cent[which], sizeof(double) * (size_t)s.dp,
                            sizeof(double) * (size_t)s.d, (size_t)s.k, hipMemcpyDeviceToHost, w->stream));
    return AS_OK;
}

// labels[out] = assign(cent[cur]) against labels[prev] (prev < 0: none), dist, the inertia partials and the changed word
as_status km_assign(const as_space* sp, KmeansWork* w, const KmShape& s, int cur, int out, int prev, const KmTimer& tm, int64_t* counts) {
    unsigned long long* stat = w->stat_d;
    AS_TRY(tm.begin());
    hipLaunchKernelGGL(km_norms_kernel, dim3((unsigned)((s.kp + 3) / 4)), dim3(256), 0, w->stream, (const double*)w->cent[cur], (double*)w->cn, stat,
                       s.k, s.kp, s.dp);
    KmAssignArgs a;
    a.x32 = sp->x32; a.x64 = sp->x64; a.n64 = sp->n64; a.cent = w->cent[cur]; a.cn = w->cn; a.labels = w->labels[out];
    a.prev = prev < 0 ? nullptr : (const int32_t*)w->labels[prev]; a.dist = w->dist; a.ipart = w->ipart; a.changed = stat;
    a.n = s.n; a.d = s.d; a.dp = s.dp; a.kp = s.kp;
    const unsigned grid = km_grid((s.n + KM_ROWS - 1) / KM_ROWS);
    if (sp->x64) hipLaunchKernelGGL(km_assign_kernel<true>, dim3(grid), dim3(256), 0, w->stream, a);
    else hipLaunchKernelGGL(km_assign_kernel<false>, dim3(grid), dim3(256), 0, w->stream, a);
    AS_HIP(hipGetLastError());
    AS_TRY(tm.end(&w->us[0]));
    counts[1] += 1;
    return AS_OK;
}

// the member list, the counts, the starts and the segment starts of labels[which]; scatter false: counts and empties alone
as_status km_order(KmeansWork* w, const KmShape& s, int which, bool scatter, const KmTimer& tm, int64_t* counts) {
    int32_t* cnt = w->counts;
    const int32_t* labels = w->labels[which];
    const size_t lds = sizeof(int32_t) * (size_t)(KM_SORT_THREADS / 64) * (size_t)s.k;
    const unsigned grid = km_grid(std::min<int64_t>((s.units + 1) / 2, (int64_t)w->cus * 8));
    AS_TRY(tm.begin());
    hipLaunchKernelGGL(km_clear_kernel, dim3((unsigned)((s.kp + 255) / 256)), dim3(256), 0, w->stream, cnt, s.kp);
    hipLaunchKernelGGL(km_hist_kernel, dim3(grid), dim3(KM_SORT_THREADS), lds, w->stream, labels, s.n, s.k, s.unit_rows, s.units, (int32_t*)w->table, cnt);
    hipLaunchKernelGGL(km_scan_kernel, dim3((unsigned)((s.k + 63) / 64)), dim3(64), 0, w->stream, (int32_t*)w->table, (const int32_t*)cnt,
                       cnt + s.kp, cnt + 2 * s.kp + 1, (unsigned long long*)w->stat_d, s.k, s.units);
    counts[2] += 3;
    if (scatter) {
        hipLaunchKernelGGL(km_scatter_kernel, dim3(grid), dim3(KM_SORT_THREADS), lds, w->stream, labels, s.n, s.k, s.unit_rows, s.units,
                           (const int32_t*)w->table, (int32_t*)w->members);
        counts[2] += 1;
    }
    AS_HIP(hipGetLastError());
    AS_TRY(tm.end(&w->us[1]));
    return AS_OK;
}

// cent[cur ^ 1] = update(cent[cur]) from the member list km_order left
as_status km_update(const as_space* sp, KmeansWork* w, const KmShape& s, int cur, const KmTimer& tm, int64_t* counts) {
    const int32_t* cnt = w->counts;
    KmUpdateArgs a;
    a.x32 = sp->x32; a.x64 = sp->x64; a.members = w->members; a.counts = cnt; a.start = cnt + s.kp; a.segstart = cnt + 2 * s.kp + 1;
    a.part = w->part; a.cent_old = w->cent[cur]; a.cent_new = w->cent[cur ^ 1]; a.d = s.d; a.dp = s.dp; a.k = s.k; a.kp = s.kp;
    const dim3 pgrid((unsigned)((s.slots + 3) / 4), (unsigned)((s.d + 63) / 64));
    AS_TRY(tm.begin());
    if (sp->x64) hipLaunchKernelGGL(km_update_part_kernel<true>, pgrid, dim3(256), 0, w->stream, a);
    else hipLaunchKernelGGL(km_update_part_kernel<false>, pgrid, dim3(256), 0, w->stream, a);
    hipLaunchKernelGGL(km_update_final_kernel, dim3((unsigned)((s.dp + 255) / 256), (unsigned)s.kp), dim3(256), 0, w->stream, a);
    AS_HIP(hipGetLastError());
    AS_TRY(tm.end(&w->us[2]));
    counts[3] += 2;
    return AS_OK;
}

// `words` of the device's words to the pinned copy: one wait
as_status km_read(KmeansWork* w, int words, int64_t* counts) {
    AS_HIP(hipMemcpyAsync((unsigned long long*)w->stat_h, (const unsigned long long*)w->stat_d, sizeof(unsigned long long) * words,
                          hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[4] += 1;
    return AS_OK;
}

as_status km_begin(const as_space* sp, int64_t k, bool order, KmeansWork** w, KmTimer* tm) {
    AS_TRY(km_work_get(sp, w));
    AS_TRY(km_reserve(*w, KmShape(sp, k), order));
    *tm = KmTimer{*w, g_kmeans_timing.load(std::memory_order_relaxed) != 0};
    for (double& v : (*w)->us) v = 0.0;
    return AS_OK;
}

as_status km_assign_run(const as_space* sp, const double* cent, int64_t k, int32_t* labels_host, double* dist_host, int64_t* counts) {
    KmeansWork* w;
    KmTimer tm{nullptr, false};
    AS_TRY(km_begin(sp, k, false, &w, &tm));
    const KmShape s(sp, k);
    AS_TRY(km_upload(w, s, 0, cent));
    AS_TRY(km_assign(sp, w, s, 0, 0, -1, tm, counts));
    AS_HIP(hipMemcpyAsync(labels_host, (const int32_t*)w->labels[0], sizeof(int32_t) * (size_t)s.n, hipMemcpyDeviceToHost, w->stream));
    if (dist_host) AS_HIP(hipMemcpyAsync(dist_host, (const double*)w->dist, sizeof(double) * (size_t)s.n, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[4] += 1;
    w->us[3] = 1.0;
    return AS_OK;
}

as_status km_update_run(const as_space* sp, const int32_t* labels_host, const double* cent, int64_t k, double* out_cent, int64_t* counts) {
    KmeansWork* w;
    KmTimer tm{nullptr, false};
    AS_TRY(km_begin(sp, k, true, &w, &tm));
    const KmShape s(sp, k);
    AS_TRY(km_upload(w, s, 0, cent));
    AS_HIP(hipMemcpyAsync((int32_t*)w->labels[0], labels_host, sizeof(int32_t) * (size_t)s.n, hipMemcpyHostToDevice, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    AS_TRY(km_order(w, s, 0, true, tm, counts));
    AS_TRY(km_update(sp, w, s, 0, tm, counts));
    AS_TRY(km_download(w, s, 1, out_cent));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[4] += 1;
    return AS_OK;
}

as_status km_lloyd_run(const as_space* sp, const KmeansCall& c, int64_t* counts) {
    KmeansWork* w;
    KmTimer tm{nullptr, false};
    AS_TRY(km_begin(sp, c.k, true, &w, &tm));
    const KmShape s(sp, c.k);
    const unsigned long long* host = w->stat_h;
    AS_TRY(km_upload(w, s, 0, c.init));
    int cur = 0, lab = 0;
    bool converged = false, ordered = false;
    int64_t t = 0;
    while (t < c.max_iters) {
        ++t;
        lab = (int)(t & 1);
        AS_TRY(km_assign(sp, w, s, cur, lab, t == 1 ? -1 : lab ^ 1, tm, counts));
        AS_TRY(km_read(w, 1, counts));
        counts[0] += 1;
        if (host[0] > (unsigned long long)s.n) {
            set_err("kmeans: the device reported %llu changed labels of %lld items", host[0], (long long)s.n);
            return AS_EHIP;
        }
        c.out_changed[t - 1] = (int64_t)host[0];
        if (host[0] == 0) {
            converged = true;
            break;
        }
        AS_TRY(km_order(w, s, lab, true, tm, counts));
        AS_TRY(km_update(sp, w, s, cur, tm, counts));
        cur ^= 1;
        ordered = true;
    }
    // the counts of the labels returned: the last ordering's unless the loop ended on an assignment
    if (converged || !ordered) AS_TRY(km_order(w, s, lab, false, tm, counts));
    hipLaunchKernelGGL(km_inertia_kernel, dim3(1), dim3(256), 0, w->stream, (const double*)w->ipart, 2 * ((s.n + KM_ROWS - 1) / KM_ROWS),
                       (unsigned long long*)w->stat_d);
    AS_HIP(hipGetLastError());
    AS_TRY(km_download(w, s, cur, c.out_centroids));
    AS_HIP(hipMemcpyAsync(c.out_labels, (const int32_t*)w->labels[lab], sizeof(int32_t) * (size_t)s.n, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipMemcpyAsync(c.out_counts32, (const int32_t*)w->counts, sizeof(int32_t) * (size_t)s.k, hipMemcpyDeviceToHost, w->stream));
    AS_TRY(km_read(w, 3, counts));
    c.info->iterations = t;
    c.info->converged = converged ? 1 : 0;
    c.info->empty = (int64_t)host[2];
    memcpy(&c.info->inertia, &host[1], sizeof(double));
    w->us[3] = (double)t;
    return AS_OK;
}

// (a failed run leaves nothing on the stream when the caller releases the lock)
template <typename F>
as_status km_guard(const as_space* sp, F&& run) {
    const as_status s = run();
    if (s != AS_OK && sp->kmeans_ws && sp->kmeans_ws->stream) (void)hipStreamSynchronize(sp->kmeans_ws->stream);
    return s;
}

}  // namespace

void set_kmeans_grid_cap(int v) { g_kmeans_grid_cap.store(v > 0 ? v : 0, std::memory_order_relaxed); }
void set_kmeans_timing(int v) { g_kmeans_timing.store(v ? 1 : 0, std::memory_order_relaxed); }
// for the seeding (as_kmeans_seed.hip), which runs on the same workspace and stream
as_status kmeans_work_get(const as_space* sp, KmeansWork** out) { return km_work_get(sp, out); }
bool kmeans_timing_on() { return g_kmeans_timing.load(std::memory_order_relaxed) != 0; }

// for the bounded loop (as_kmeans_bounded.hip): the buffers and the launches of the loop above, as they are
int kmeans_loop_kp(int64_t k) { return (int)((k + KM_C - 1) / KM_C * KM_C); }
as_status kmeans_loop_begin(const as_space* sp, int64_t k, bool order, KmeansWork** w) {
    KmTimer tm{nullptr, false};
    return km_begin(sp, k, order, w, &tm);
}
as_status kmeans_loop_upload(const as_space* sp, KmeansWork* w, int64_t k, int which, const double* host) { return km_upload(w, KmShape(sp, k), which, host); }
as_status kmeans_loop_download(const as_space* sp, KmeansWork* w, int64_t k, int which, double* host) { return km_download(w, KmShape(sp, k), which, host); }
as_status kmeans_loop_norms(const as_space* sp, KmeansWork* w, int64_t k, int cur) {
    const KmShape s(sp, k);
    hipLaunchKernelGGL(km_norms_kernel, dim3((unsigned)((s.kp + 3) / 4)), dim3(256), 0, w->stream, (const double*)w->cent[cur], (double*)w->cn,
                       (unsigned long long*)w->stat_d, s.k, s.kp, s.dp);
    AS_HIP(hipGetLastError());
    return AS_OK;
}
as_status kmeans_loop_order(const as_space* sp, KmeansWork* w, int64_t k, int which, bool scatter, int64_t* counts) {
    return km_order(w, KmShape(sp, k), which, scatter, KmTimer{w, kmeans_timing_on()}, counts);
}
as_status kmeans_loop_update(const as_space* sp, KmeansWork* w, int64_t k, int cur, int64_t* counts) {
    return km_update(sp, w, KmShape(sp, k), cur, KmTimer{w, kmeans_timing_on()}, counts);
}
as_status kmeans_loop_read(KmeansWork* w, int words, int64_t* counts) { return km_read(w, words, counts); }
unsigned kmeans_loop_grid(int64_t blocks) { return km_grid(blocks); }
as_status kmeans_loop_inertia(const as_space* sp, KmeansWork* w) {
    hipLaunchKernelGGL(km_inertia_kernel, dim3(1), dim3(256), 0, w->stream, (const double*)w->ipart, 2 * ((sp->n + KM_ROWS - 1) / KM_ROWS),
                       (unsigned long long*)w->stat_d);
    AS_HIP(hipGetLastError());
    return AS_OK;
}

void kmeans_work_free(KmeansWork* w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;   // (the buffers and the events free themselves)
}

double kmeans_kernel_us(const KmeansWork* w, int part) { return w && part >= 0 && part < 4 ? w->us[part] : 0.0; }

as_status kmeans_assign(const as_space* sp, const double* cent, int64_t k, int32_t* labels_host, double* dist_host, int64_t* counts) {
    return km_guard(sp, [&] { return km_assign_run(sp, cent, k, labels_host, dist_host, counts); });
}
as_status kmeans_update(const as_space* sp, const int32_t* labels_host, const double* cent, int64_t k, double* out_cent, int64_t* counts) {
    return km_guard(sp, [&] { return km_update_run(sp, labels_host, cent, k, out_cent, counts); });
}
as_status kmeans_lloyd(const as_space* sp, const KmeansCall& c, int64_t* counts) {
    return km_guard(sp, [&] { return km_lloyd_run(sp, c, counts); });
}

}  // namespace as
