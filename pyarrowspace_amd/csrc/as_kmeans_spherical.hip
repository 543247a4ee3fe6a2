// Spherical (cosine) k-means over the items (section 5.31).  Items are the stored items, as in as_kmeans.hip;
// a row's scale is w_i = fl(1 / fl(sqrt(n64[i]))), NaN on a DEAD row (n64 of 0, NaN or inf, or a w that is not finite); centroids are
// k <= 4096 UNIT rows of d doubles on the device, [kp][dp], zero padded.
//   UNIT     kms_unit_kernel, a wave per centroid row, in place: lane l adds fl(v_c v_c) over c = l, l + 64, .. in ascending order
//            (product and add rounded separately), the halving tree s_l += s_{l + o}, o = 32 .. 1, leaves q in lane 0; r = fl(1 /
//            fl(sqrt(q))); v_c <- fl(v_c r).  A row with no direction (q of 0, NaN or inf, r not finite) and the row of an empty
//            cluster take the old centroid's row instead.  Pad rows (j >= k) stay zero and are never read as centroids: the assign
//            kernel carries k in its arguments and leaves every j >= k out by index.  Clears the changed-labels word.
//   ASSIGN   kms_assign_kernel: km_assign_kernel's fp64 GEMM on v_mfma_f64_16x16x4_f64 -- the same 128 x 64 x 32 tile, the same LDS
//            pitch, the same staging and operand layouts, the same ascending order of the columns in every accumulator -- with an
//            epilogue of its own: the key of (i, j) is the dot g itself, the LARGER wins, ties go to the smaller j, a NaN never
//            wins; no centroid-norm load.  After the last tile the four lane groups of a row meet by cross-lane moves, the two
//            waves that share rows through LDS, and the owning lane reads w: label (-1 on a dead row or without a comparable g),
//            cos = min(1, max(-1, fl(g w))), the count of changed labels (one integer atomic per wave), the cohesion partial of
//            its 64 rows (a fixed __shfl_down tree).  The grid strides over the row tiles ("kmeans_grid_cap").
//   UPDATE   pinned in bits given the labels and w: kms_update_part_kernel, a wave per (segment slot, 64-column slab), adds y_m =
//            fl(x_m w_m) of the members [256 s, 256 s + 256) of a cluster one by one in ascending id from the first one's y row,
//            eight gathered loads in flight before eight ordered adds; kms_update_final_kernel adds the segment sums in order into
//            the new centroid buffer; UNIT then runs over it.  There is no division by the count.
// The member ordering is the counting sort of as_kmeans.hip (kmeans_loop_order), the buffers and the stream are the space's k-means
// workspace.  The Lloyd loop reads one pinned word per iteration.  Entry points: as_api.hip (as_kmeans_cos_assign,
// as_kmeans_spherical, as_kmeans_spherical_update, as_kmeans_spherical_scales, as_kmeans_spherical_counters,
// as_kmeans_spherical_kernel_us).
#include <algorithm>
#include <cmath>
#include <limits>

#include "as_common.hpp"

// S28 rounds every product and every sum once: no multiply of this file may be fused with the add behind it (HIP's __dmul_rn /
// __dadd_rn are plain operators of a header compiled with contraction on: see as_diffuse.hip)
#pragma clang fp contract(off)

namespace as {

namespace {

typedef float ks_f32x2 __attribute__((ext_vector_type(2)));
typedef float ks_f32x4 __attribute__((ext_vector_type(4)));
typedef double ks_f64x2 __attribute__((ext_vector_type(2)));
typedef double ks_f64x4 __attribute__((ext_vector_type(4)));

constexpr int KS_ROWS = 128;   // the tile of km_assign_kernel: rows of a block,
constexpr int KS_C = 64;       // centroids of a tile (kp is a multiple of it),
constexpr int KS_K = 32;       // columns of a K stage (dp is a multiple of it)
constexpr int KS_P = KS_K + 2;
constexpr int KS_SEG = 256;    // members of an update segment: part of the definition (S25, S28)
constexpr int KS_NONE = 0x7fffffff;

__device__ __forceinline__ double ks_inf() { return __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ double ks_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
// the larger dot wins, ties go to the smaller j; a NaN compares false both ways and never enters
__device__ __forceinline__ bool ks_better(double ga, int ja, double gb, int jb) { return ga > gb || (ga == gb && ja < jb); }
// fl(1 / fl(sqrt(q))), NaN where q is 0, NaN, inf or negative or the result is not finite
__device__ __forceinline__ double ks_rsqrt(double q) {
    if (!(q > 0.0) || !(q < ks_inf())) return ks_nan();
    const double r = 1.0 / sqrt(q);
    return r < ks_inf() ? r : ks_nan();
}

// w[i] = the row scale, a thread per row
__global__ __launch_bounds__(256) void kms_scale_kernel(const double* __restrict__ n64, double* __restrict__ w, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) w[i] = ks_rsqrt(n64[i]);
}

// cent[j] <- unit(cent[j]), a wave per row j < k; q[j] = its squared length.  counts (may be null): a cluster with no member keeps
// the row the final kernel copied from `old`; old (may be null): a row with no direction takes old's row, without it stays as it is.
__global__ __launch_bounds__(256) void kms_unit_kernel(double* __restrict__ cent, const double* __restrict__ old, const int32_t* __restrict__ counts,
                                                       double* __restrict__ q, unsigned long long* stat, int k, int64_t dp) {
    if (blockIdx.x == 0 && threadIdx.x == 0) stat[0] = 0ull;
    const int lane = lane_id(), j = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (j >= k) return;
    double* v = cent + (int64_t)j * dp;
    if (counts && counts[j] == 0) {
        if (lane == 0) q[j] = 0.0;
        return;
    }
    double s = 0.0;
    for (int64_t c = lane; c < dp; c += 64) {
        const double e = v[c];
        s = s + e * e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_down(s, o, 64);
    s = __shfl(s, 0, 64);
    const double r = ks_rsqrt(s);
    if (lane == 0) q[j] = s;
    if (r == r) {
        for (int64_t c = lane; c < dp; c += 64) v[c] = v[c] * r;
    } else if (old) {
        for (int64_t c = lane; c < dp; c += 64) v[c] = old[(int64_t)j * dp + c];
    }
}

struct KmsAssignArgs {
    const float* x32;
    const double* x64;
    const double* w;      // [n] the row scales; NaN: a dead row
    const double* cent;   // [kp][dp] unit rows, the rows j >= k zero
    int32_t* labels;      // [n]
    const int32_t* prev;  // [n] the labels before; null: every label >= 0 counts as changed
    double* cosv;         // [n]
    double* ipart;        // [2 tiles] the cohesion partials of 64 rows each
    unsigned long long* changed;
    int64_t n, d, dp;
    int k, kp;
};

// (two blocks per CU, as km_assign_kernel: see the register counts in DESIGN.md section 5.31)
template <bool F64>
__global__ __launch_bounds__(256, 2) void kms_assign_kernel(KmsAssignArgs a) {
    constexpr int NR = F64 ? 16 : 4;   // rows a thread stages per K stage
    __shared__ __attribute__((aligned(16))) double cs[KS_C * KS_P];
    __shared__ __attribute__((aligned(16))) char xs_raw[KS_ROWS * KS_P * (F64 ? 8 : 4)];
    __shared__ double s_key[KS_ROWS];
    __shared__ int s_j[KS_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
    const int lk = lane >> 4, lc = lane & 15;
    // staging maps and operand layouts: km_assign_kernel (as_kmeans.hip)
    const int xc = F64 ? (tid & 31) : (tid & 7) * 4, xr = F64 ? (tid >> 5) : (tid >> 3), xstep = F64 ? 8 : 32;
    const int qc = (tid & 15) * 2, qr = tid >> 4;
    const int64_t ld = F64 ? a.d : a.dp;
    const int64_t tiles = (a.n + KS_ROWS - 1) / KS_ROWS;
    const int64_t stages = (int64_t)(a.kp / KS_C) * (a.dp / KS_K);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * KS_ROWS;
        ks_f32x4 vf[F64 ? 1 : NR];
        double vd[F64 ? NR : 1];
        ks_f64x2 vq[4];
        auto load_stage = [&](int c0, int64_t k0) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int64_t pos = row0 + xr + xstep * i;
                if constexpr (F64) vd[i] = (pos < a.n && k0 + xc < a.d) ? a.x64[pos * ld + k0 + xc] : 0.0;
                else vf[i] = pos < a.n ? *(const ks_f32x4*)(a.x32 + pos * ld + k0 + xc) : ks_f32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) vq[i] = *(const ks_f64x2*)(a.cent + (int64_t)(c0 + qr + 16 * i) * a.dp + k0 + qc);
        };
        double bk[4];
        int bj[4];
        ks_f64x4 acc[2][4];
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            bk[jb] = -ks_inf();
            bj[jb] = KS_NONE;
#pragma unroll
            for (int ib = 0; ib < 2; ++ib) acc[ib][jb] = ks_f64x4{0.0, 0.0, 0.0, 0.0};
        }
        int c0 = 0;
        int64_t k0 = 0;
        load_stage(0, 0);
        for (int64_t s = 0; s < stages; ++s) {
            __syncthreads();   // the previous stage has been consumed
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                if constexpr (F64) ((double*)xs_raw)[(xr + xstep * i) * KS_P + xc] = vd[i];
                else {
                    ks_f32x2* dst = (ks_f32x2*)((float*)xs_raw + (xr + xstep * i) * KS_P + xc);
                    dst[0] = ks_f32x2{vf[i][0], vf[i][1]};
                    dst[1] = ks_f32x2{vf[i][2], vf[i][3]};
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) *(ks_f64x2*)(cs + (qr + 16 * i) * KS_P + qc) = vq[i];
            __syncthreads();
            int nc0 = c0;
            int64_t nk0 = k0 + KS_K;
            if (nk0 >= a.dp) {   // the next stage opens the next centroid tile
                nk0 = 0;
                nc0 += KS_C;
            }
            if (s + 1 < stages) load_stage(nc0, nk0);   // in flight under the MFMAs below
#pragma unroll
            for (int ks = 0; ks < KS_K / 4; ++ks) {
                double av[2], bv[4];
#pragma unroll
                for (int ib = 0; ib < 2; ++ib) av[ib] = cs[(32 * wj + 16 * ib + lc) * KS_P + 4 * ks + lk];
#pragma unroll
                for (int jb = 0; jb < 4; ++jb) {
                    const int e = (64 * wi + 16 * jb + lc) * KS_P + 4 * ks + lk;
                    bv[jb] = F64 ? ((const double*)xs_raw)[e] : (double)((const float*)xs_raw)[e];
                }
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb) acc[ib][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ib], bv[jb], acc[ib][jb], 0, 0, 0);
            }
            if (nk0 == 0) {
                // the tile's dots are complete.  C/D: col = lane & 15 (the row of block jb), row = (lane >> 4) + 4 reg (the centroid).
                // j ascends with (ib, r) within a lane, so a strict > keeps the smaller j of a tie; pad centroids leave by index
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = c0 + 32 * wj + 16 * ib + lk + 4 * r;
                        if (j < a.k) {
#pragma unroll
                            for (int jb = 0; jb < 4; ++jb) {
                                const double g = acc[ib][jb][r];
                                if (ks_better(g, j, bk[jb], bj[jb])) {
                                    bk[jb] = g;
                                    bj[jb] = j;
                                }
                            }
                        }
                    }
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb) acc[ib][jb] = ks_f64x4{0.0, 0.0, 0.0, 0.0};
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
                if (ks_better(ok, oj, bk[jb], bj[jb])) {
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
            if (ks_better(ok, oj, mk, mj)) {
                mk = ok;
                mj = oj;
            }
            const int64_t row = row0 + 64 * wi + lane;
            const bool live = row < a.n;
            int label = -1;
            double cv = ks_nan();
            bool ch = false;
            if (live) {
                const double ws = a.w[row];
                if (ws == ws && mj != KS_NONE) {
                    label = mj;
                    cv = mk * ws;
                    cv = cv < -1.0 ? -1.0 : cv;
                    cv = cv > 1.0 ? 1.0 : cv;
                    ch = a.prev ? a.prev[row] != label : true;
                }
                a.labels[row] = label;
                a.cosv[row] = cv;
            }
            const int nch = __popcll(__ballot(ch));
            if (lane == 0 && nch) atomicAdd(a.changed, (unsigned long long)nch);
            double v = label >= 0 ? cv : 0.0;   // the cohesion partial of these 64 rows: a fixed halving tree
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);
            if (lane == 0) a.ipart[tile * 2 + wi] = v;
        }
    }
}

struct KmsUpdateArgs {
    const float* x32;
    const double* x64;
    const double* w;           // [n]
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

// A wave per (segment slot, 64-column slab), as km_update_part_kernel: the slot's cluster by bisection of segstart, its members' rows
// times their scales added in order.
template <bool F64>
__global__ __launch_bounds__(256) void kms_update_part_kernel(KmsUpdateArgs a) {
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
    const int32_t* mem = a.members + a.start[lo] + KS_SEG * seg;
    const int m = min(KS_SEG, a.counts[lo] - KS_SEG * seg);
    const int64_t col = (int64_t)blockIdx.y * 64 + lane;
    if (col >= a.d) return;
    double acc = 0.0;
    for (int t = 0; t < m; t += 8) {
        double v[8], ws[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t id = mem[min(t + u, m - 1)];
            v[u] = F64 ? a.x64[id * a.d + col] : (double)a.x32[id * a.dp + col];
            ws[u] = a.w[id];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double y = v[u] * ws[u];
            if (t + u < m) acc = t + u == 0 ? y : acc + y;
        }
    }
    a.part[(int64_t)slot * a.dp + col] = acc;
}

// T_j = P_0 + P_1 + .. in that order, a thread per (cluster, column); an empty cluster, a pad row and a pad column take what the old
// buffer held.  kms_unit_kernel runs behind it.
__global__ __launch_bounds__(256) void kms_update_final_kernel(KmsUpdateArgs a) {
    const int j = blockIdx.y;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= a.dp) return;
    double out = a.cent_old[(int64_t)j * a.dp + col];
    if (j < a.k && col < a.d && a.counts[j] > 0) {
        const int s0 = a.segstart[j], ns = a.segstart[j + 1] - s0;
        out = a.part[(int64_t)s0 * a.dp + col];
        for (int s = 1; s < ns; ++s) out = out + a.part[(int64_t)(s0 + s) * a.dp + col];
    }
    a.cent_new[(int64_t)j * a.dp + col] = out;
}

// ------------------------------------------------------------------ host side
struct KmsShape {
    int64_t n, d, dp;
    int k, kp;
    int64_t slots;
    KmsShape(const as_space* sp, int64_t k_) : n(sp->n), d(sp->d), dp(sp->dp), k((int)k_), kp(kmeans_loop_kp(k_)) {
        slots = n / KS_SEG + k + 1;   // sum_j ceil(count_j / 256) <= n / 256 + k: what kmeans_loop_begin reserved for
    }
};

// one timed part: launch() between two events on the work's stream, added to us[part] (timing waits for it)
template <typename F>
as_status kms_timed(KmeansWork* w, int part, F&& launch) {
    const bool on = kmeans_timing_on();
    if (on) AS_HIP(hipEventRecord(w->ev.e[0], w->stream));
    launch();
    AS_HIP(hipGetLastError());
    if (!on) return AS_OK;
    AS_HIP(hipEventRecord(w->ev.e[1], w->stream));
    AS_HIP(hipEventSynchronize(w->ev.e[1]));
    float ms = 0.0f;
    AS_HIP(hipEventElapsedTime(&ms, w->ev.e[0], w->ev.e[1]));
    w->spherical.us[part] += (double)ms * 1e3;
    return AS_OK;
}

// the workspace of a call: the loop's buffers, q, and w of every row (one launch per call)
as_status kms_begin(const as_space* sp, int64_t k, bool order, KmeansWork** out, int64_t* counts) {
    AS_TRY(kmeans_loop_begin(sp, k, order, out));
    KmeansWork* w = *out;
    KmsWork& b = w->spherical;
    AS_TRY(reserve_or_err(b.w, sp->n, "kmeans_spherical row scales"));
    AS_TRY(reserve_or_err(b.q, kmeans_loop_kp(k), "kmeans_spherical centroid lengths"));
    for (double& v : b.us) v = 0.0;
    hipLaunchKernelGGL(kms_scale_kernel, dim3((unsigned)((sp->n + 255) / 256)), dim3(256), 0, w->stream, (const double*)sp->n64, (double*)b.w, sp->n);
    AS_HIP(hipGetLastError());
    counts[6] += 1;
    return AS_OK;
}

// cent[which] <- unit of its rows; old < 0: no old buffer; by_counts: the clusters without a member keep their rows
as_status kms_unit(KmeansWork* w, const KmsShape& s, int which, int old, bool by_counts, int64_t* counts) {
    AS_TRY(kms_timed(w, 0, [&] {
        hipLaunchKernelGGL(kms_unit_kernel, dim3((unsigned)((s.k + 3) / 4)), dim3(256), 0, w->stream, (double*)w->cent[which],
                           old < 0 ? (const double*)nullptr : (const double*)w->cent[old], by_counts ? (const int32_t*)w->counts : (const int32_t*)nullptr,
                           (double*)w->spherical.q, (unsigned long long*)w->stat_d, s.k, s.dp);
    }));
    counts[5] += 1;
    return AS_OK;
}

// labels[out] = assign(cent[cur]) against labels[prev] (prev < 0: none), the cosines into dist, the cohesion partials, the changed word
as_status kms_assign(const as_space* sp, KmeansWork* w, const KmsShape& s, int cur, int out, int prev, int64_t* counts) {
    KmsAssignArgs a;
    a.x32 = sp->x32; a.x64 = sp->x64; a.w = w->spherical.w; a.cent = w->cent[cur]; a.labels = w->labels[out];
    a.prev = prev < 0 ? nullptr : (const int32_t*)w->labels[prev]; a.cosv = w->dist; a.ipart = w->ipart; a.changed = w->stat_d;
    a.n = s.n; a.d = s.d; a.dp = s.dp; a.k = s.k; a.kp = s.kp;
    const unsigned grid = kmeans_loop_grid((s.n + KS_ROWS - 1) / KS_ROWS);
    AS_TRY(kms_timed(w, 1, [&] {
        if (sp->x64) hipLaunchKernelGGL(kms_assign_kernel<true>, dim3(grid), dim3(256), 0, w->stream, a);
        else hipLaunchKernelGGL(kms_assign_kernel<false>, dim3(grid), dim3(256), 0, w->stream, a);
    }));
    counts[1] += 1;
    return AS_OK;
}

// cent[cur ^ 1] = update(cent[cur]) from the member list kmeans_loop_order left, unit rows
as_status kms_update(const as_space* sp, KmeansWork* w, const KmsShape& s, int cur, int64_t* counts) {
    const int32_t* cnt = w->counts;
    KmsUpdateArgs a;
    a.x32 = sp->x32; a.x64 = sp->x64; a.w = w->spherical.w; a.members = w->members; a.counts = cnt; a.start = cnt + s.kp;
    a.segstart = cnt + 2 * s.kp + 1; a.part = w->part; a.cent_old = w->cent[cur]; a.cent_new = w->cent[cur ^ 1]; a.d = s.d; a.dp = s.dp;
    a.k = s.k; a.kp = s.kp;
    const dim3 pgrid((unsigned)((s.slots + 3) / 4), (unsigned)((s.d + 63) / 64));
    AS_TRY(kms_timed(w, 3, [&] {
        if (sp->x64) hipLaunchKernelGGL(kms_update_part_kernel<true>, pgrid, dim3(256), 0, w->stream, a);
        else hipLaunchKernelGGL(kms_update_part_kernel<false>, pgrid, dim3(256), 0, w->stream, a);
        hipLaunchKernelGGL(kms_update_final_kernel, dim3((unsigned)((s.dp + 255) / 256), (unsigned)s.kp), dim3(256), 0, w->stream, a);
    }));
    counts[3] += 2;
    return kms_unit(w, s, cur ^ 1, cur, true, counts);
}

as_status kms_assign_run(const as_space* sp, const double* cent, int64_t k, int32_t* labels_host, double* cos_host, int64_t* counts) {
    KmeansWork* w;
    AS_TRY(kms_begin(sp, k, false, &w, counts));
    const KmsShape s(sp, k);
    AS_TRY(kmeans_loop_upload(sp, w, k, 0, cent));
    AS_TRY(kms_unit(w, s, 0, -1, false, counts));
    AS_TRY(kms_assign(sp, w, s, 0, 0, -1, counts));
    AS_HIP(hipMemcpyAsync(labels_host, (const int32_t*)w->labels[0], sizeof(int32_t) * (size_t)s.n, hipMemcpyDeviceToHost, w->stream));
    if (cos_host) AS_HIP(hipMemcpyAsync(cos_host, (const double*)w->dist, sizeof(double) * (size_t)s.n, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[4] += 1;
    w->spherical.us[4] = 1.0;
    return AS_OK;
}

as_status kms_update_run(const as_space* sp, const int32_t* labels_host, const double* cent, int64_t k, double* out_cent, int64_t* counts) {
    KmeansWork* w;
    AS_TRY(kms_begin(sp, k, true, &w, counts));
    const KmsShape s(sp, k);
    AS_HIP(hipMemcpyAsync((int32_t*)w->labels[0], labels_host, sizeof(int32_t) * (size_t)s.n, hipMemcpyHostToDevice, w->stream));
    AS_TRY(kmeans_loop_upload(sp, w, k, 0, cent));   // (waits: the labels have crossed too)
    AS_TRY(kmeans_loop_order(sp, w, k, 0, true, counts));
    AS_TRY(kms_update(sp, w, s, 0, counts));
    AS_TRY(kmeans_loop_download(sp, w, k, 1, out_cent));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[4] += 1;
    return AS_OK;
}

as_status kms_scales_run(const as_space* sp, double* out_w, int64_t* counts) {
    KmeansWork* w;
    AS_TRY(kms_begin(sp, 1, false, &w, counts));
    AS_HIP(hipMemcpyAsync(out_w, (const double*)w->spherical.w, sizeof(double) * (size_t)sp->n, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[4] += 1;
    return AS_OK;
}

as_status kms_lloyd_run(const as_space* sp, const KmeansCall& c, int64_t* counts) {
    KmeansWork* w;
    AS_TRY(kms_begin(sp, c.k, true, &w, counts));
    const KmsShape s(sp, c.k);
    const unsigned long long* host = w->stat_h;
    AS_TRY(kmeans_loop_upload(sp, w, c.k, 0, c.init));
    AS_TRY(kms_unit(w, s, 0, -1, false, counts));
    int cur = 0, lab = 0;
    bool converged = false, ordered = false;
    int64_t t = 0;
    while (t < c.max_iters) {
        ++t;
        lab = (int)(t & 1);
        AS_TRY(kms_assign(sp, w, s, cur, lab, t == 1 ? -1 : lab ^ 1, counts));
        AS_TRY(kmeans_loop_read(w, 1, counts));
        counts[0] += 1;
        if (host[0] > (unsigned long long)s.n) {
            set_err("kmeans_spherical: the device reported %llu changed labels of %lld items", host[0], (long long)s.n);
            return AS_EHIP;
        }
        c.out_changed[t - 1] = (int64_t)host[0];
        if (host[0] == 0) {
            converged = true;
            break;
        }
        AS_TRY(kmeans_loop_order(sp, w, c.k, lab, true, counts));
        AS_TRY(kms_update(sp, w, s, cur, counts));   // (its unit launch clears the changed word for the next assignment)
        cur ^= 1;
        ordered = true;
    }
    // the counts of the labels returned: the last ordering's unless the loop ended on an assignment (as kmeans_lloyd)
    if (converged || !ordered) AS_TRY(kmeans_loop_order(sp, w, c.k, lab, false, counts));
    AS_TRY(kmeans_loop_inertia(sp, w));
    AS_TRY(kmeans_loop_download(sp, w, c.k, cur, c.out_centroids));
    AS_HIP(hipMemcpyAsync(c.out_labels, (const int32_t*)w->labels[lab], sizeof(int32_t) * (size_t)s.n, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipMemcpyAsync(c.out_counts32, (const int32_t*)w->counts, sizeof(int32_t) * (size_t)s.k, hipMemcpyDeviceToHost, w->stream));
    AS_TRY(kmeans_loop_read(w, 3, counts));
    c.info->iterations = t;
    c.info->converged = converged ? 1 : 0;
    c.info->empty = (int64_t)host[2];
    memcpy(&c.info->inertia, &host[1], sizeof(double));
    w->spherical.us[4] = (double)t;
    return AS_OK;
}

// (a failed run leaves nothing on the stream when the caller releases the lock)
template <typename F>
as_status kms_guard(const as_space* sp, F&& run) {
    const as_status s = run();
    if (s != AS_OK && sp->kmeans_ws && sp->kmeans_ws->stream) (void)hipStreamSynchronize(sp->kmeans_ws->stream);
    return s;
}

}  // namespace

// parts: 0 unit launches, 1 assign launches, 2 ordering launches (timed by as_kmeans.hip's own record), 3 update launches, 4 iterations
double kmeans_spherical_kernel_us(const KmeansWork* w, int part) {
    if (!w || part < 0 || part > 4) return 0.0;
    return part == 2 ? kmeans_kernel_us(w, 1) : w->spherical.us[part];
}

// for the bounded spherical loop (as_kmeans_spherical_bounded.hip): the workspace with its row scales, the unit launch and the update
// launches of the loop above, as they are
as_status kmeans_spherical_loop_begin(const as_space* sp, int64_t k, bool order, KmeansWork** w, int64_t* counts) { return kms_begin(sp, k, order, w, counts); }
as_status kmeans_spherical_loop_unit(const as_space* sp, KmeansWork* w, int64_t k, int which, int old, bool by_counts, int64_t* counts) {
    return kms_unit(w, KmsShape(sp, k), which, old, by_counts, counts);
}
as_status kmeans_spherical_loop_update(const as_space* sp, KmeansWork* w, int64_t k, int cur, int64_t* counts) {
    return kms_update(sp, w, KmsShape(sp, k), cur, counts);
}

as_status kmeans_cos_assign(const as_space* sp, const double* cent, int64_t k, int32_t* labels_host, double* cos_host, int64_t* counts) {
    return kms_guard(sp, [&] { return kms_assign_run(sp, cent, k, labels_host, cos_host, counts); });
}
as_status kmeans_spherical(const as_space* sp, const KmeansCall& c, int64_t* counts) {
    return kms_guard(sp, [&] { return kms_lloyd_run(sp, c, counts); });
}
as_status kmeans_spherical_update(const as_space* sp, const int32_t* labels_host, const double* cent, int64_t k, double* out_cent, int64_t* counts) {
    return kms_guard(sp, [&] { return kms_update_run(sp, labels_host, cent, k, out_cent, counts); });
}
as_status kmeans_spherical_scales(const as_space* sp, double* out_w, int64_t* counts) {
    return kms_guard(sp, [&] { return kms_scales_run(sp, out_w, counts); });
}

}  // namespace as
