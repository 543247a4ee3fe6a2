// Greedy k-means++ seeding over the items (section 5.29).  Every pick costs ONE pass over the stored rows,
// whatever the number L <= 16 of candidates a step tries: the candidates are the one 16-wide tile of v_mfma_f64_16x16x4_f64.
//   DIST     kseed_dist_kernel: a block of 4 waves owns one SEGMENT of 256 consecutive rows (the segment of S26's potential) and the
//            grid strides over the segments ("kmeans_seed_grid_cap").  The candidates' rows are read BY ID from the item buffer, the
//            ids from a device word array the pick kernel of the step before wrote: in K stages through LDS next to the segment's
//            rows (operand and staging layouts of km_assign_kernel, as_kmeans.hip; 32 columns a stage on fp32 rows, 16 on fp64 rows,
//            whose tile of 256 rows would not fit at 32).  A wave holds 4 row blocks x 16 candidates in 16 accumulators.  At entry
//            the block commits the step before: m[i] = G[i][l*] with l* a device word; at the end every lane turns its dots into
//            d(i, c_l) = max(0, fl(n64[i] + fl(n64[c_l] - fl(2 dot)))) and g = min(m[i], d) (a NaN d: 0 for good; the candidate's own
//            row: +0.0; a row past n: 0), the tile of g goes through LDS (aliasing the row stage) to G [rows][16] in full lines, and
//            the same LDS tile is folded by the fixed halving tree of S26 into the 16 segment sums P[s][.].  Pad candidates carry
//            n64 = NaN: their column is 0.  The first pick is the same kernel with one live candidate and m = +inf.
//   PICK     kseed_pick_kernel, one block: 16 lanes of wave 0 run the 16 serial ascending prefixes T[s][l] = T[s - 1][l] + P[s][l] side
//            by side out of LDS, chunks of 128 segments that the other three waves fetch one chunk ahead (the chain never waits for
//            memory); wave 0 chooses l* (the smallest potential, ties to the smallest l) and publishes l*, ids[t], phi[t]; then,
//            for the next step, one thread per uniform bisects T[.][l*] for its segment, and the four waves take the uniforms in
//            turn: 64 lanes fetch the segment's column of G into LDS, lane 0 walks it row by row.  The next candidates' ids are
//            left in the device word array.  A potential of 0 raises the degenerate word: the distance launches behind it return
//            at once and the pick launches fill in the smallest ids not yet marked as chosen.
// 2 k launches back to back on the k-means stream of the space, one host wait for the answer.  Entry points: as_api.hip
// (as_kmeans_seed, as_kmeans_seed_counters, as_kmeans_seed_kernel_us).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>

#include "as_common.hpp"

namespace as {

namespace {

typedef float ks_f32x2 __attribute__((ext_vector_type(2)));
typedef float ks_f32x4 __attribute__((ext_vector_type(4)));
typedef double ks_f64x4 __attribute__((ext_vector_type(4)));

constexpr int KS_SEG = 256;      // rows of a block's tile and of a segment of the potential: part of the definition (S26)
constexpr int KS_L = 16;         // candidates of a step at most: one B tile
constexpr int KS_GP = KS_L + 1;  // pitch of the tile of g in LDS, doubles
constexpr int KS_PC = 128;       // segments of a chunk of the pick kernel's prefix
// state words of a call
constexpr int KS_LSTAR = 0, KS_DEGEN = 1, KS_CURSOR = 2, KS_FILLED = 3, KS_WORDS = 4;

struct KseedDistArgs {
    const float* x32;
    const double* x64;
    const double* n64;
    const int32_t* cand;    // [16] this step's candidate ids, -1 on the pads
    const int32_t* state;
    double* G;              // [segments * 256][16]
    double* P;              // [segments][16]
    int64_t n, d, dp;
    int first;              // 1: no step before this one, m = +inf
};

template <bool F64>
__global__ __launch_bounds__(256, 2) void kseed_dist_kernel(KseedDistArgs a) {
    constexpr int KC = F64 ? 16 : 32;   // columns of a K stage
    constexpr int KP = KC + 2;          // pitch of a staged row, elements (the bank argument of as_subset.hip)
    constexpr int NR = F64 ? 16 : 8;    // rows a thread stages per K stage
    constexpr int XS_BYTES = KS_SEG * KP * (F64 ? 8 : 4), GS_BYTES = KS_SEG * KS_GP * 8;
    __shared__ __attribute__((aligned(16))) char raw[XS_BYTES > GS_BYTES ? XS_BYTES : GS_BYTES];   // the row stage, then the tile of g
    __shared__ __attribute__((aligned(16))) double cs[KS_L * KP];
    __shared__ double ms[KS_SEG];
    __shared__ double s_cn[KS_L];
    __shared__ int s_id[KS_L];
    if (a.state[KS_DEGEN]) return;   // (every block reads the same word: only pick launches write it)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lk = lane >> 4, lc = lane & 15;
    double* gs = (double*)raw;
    if (tid < KS_L) {
        const int id = a.cand[tid];
        s_id[tid] = id;
        s_cn[tid] = id >= 0 ? a.n64[id] : __longlong_as_double(0x7ff8000000000000LL);
    }
    __syncthreads();
    const int lstar = a.state[KS_LSTAR];
    // staging maps.  fp32 rows: thread t holds floats 4 (t & 7) .. + 3 of rows (t >> 3) + 32 i; fp64 rows: double t & 15 of rows
    // (t >> 4) + 16 i.  Candidates, by id: the same map on rows 0 .. 15 (fp32: threads below 128; fp64: every thread one double)
    const int xc = F64 ? (tid & 15) : (tid & 7) * 4, xr = F64 ? (tid >> 4) : (tid >> 3), xstep = F64 ? 16 : 32;
    const int64_t cid = (F64 || tid < 128) ? s_id[xr & 15] : -1;
    const int64_t segs = (a.n + KS_SEG - 1) / KS_SEG, stages = a.dp / KC;
    for (int64_t seg = blockIdx.x; seg < segs; seg += gridDim.x) {
        const int64_t row0 = seg * KS_SEG;
        ms[tid] = a.first ? key_traits<double>::inf() : a.G[(row0 + tid) * KS_L + lstar];   // the commit of the step before
        ks_f32x4 vf[F64 ? 1 : NR], qf = ks_f32x4{0, 0, 0, 0};
        double vd[F64 ? NR : 1], qd = 0.0;
        auto load_stage = [&](int64_t k0) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int64_t pos = row0 + xr + xstep * i;
                if constexpr (F64) vd[i] = (pos < a.n && k0 + xc < a.d) ? a.x64[pos * a.d + k0 + xc] : 0.0;
                else vf[i] = pos < a.n ? *(const ks_f32x4*)(a.x32 + pos * a.dp + k0 + xc) : ks_f32x4{0, 0, 0, 0};
            }
            if constexpr (F64) qd = (cid >= 0 && k0 + xc < a.d) ? a.x64[cid * a.d + k0 + xc] : 0.0;
            else qf = cid >= 0 ? *(const ks_f32x4*)(a.x32 + cid * a.dp + k0 + xc) : ks_f32x4{0, 0, 0, 0};
        };
        ks_f64x4 acc[4];
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) acc[jb] = ks_f64x4{0.0, 0.0, 0.0, 0.0};
        load_stage(0);
        for (int64_t s = 0; s < stages; ++s) {
            __syncthreads();   // the previous stage (or the previous segment's tile of g) has been consumed
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                if constexpr (F64) ((double*)raw)[(xr + xstep * i) * KP + xc] = vd[i];
                else {
                    ks_f32x2* dst = (ks_f32x2*)((float*)raw + (xr + xstep * i) * KP + xc);
                    dst[0] = ks_f32x2{vf[i][0], vf[i][1]};
                    dst[1] = ks_f32x2{vf[i][2], vf[i][3]};
                }
            }
            if constexpr (F64) cs[xr * KP + xc] = qd;
            else if (tid < 128) {
#pragma unroll
                for (int e = 0; e < 4; ++e) cs[xr * KP + xc + e] = (double)qf[e];
            }
            __syncthreads();
            if (s + 1 < stages) load_stage((s + 1) * KC);   // in flight under the MFMAs below
#pragma unroll
            for (int ks = 0; ks < KC / 4; ++ks) {
                const double av = cs[lc * KP + 4 * ks + lk];
                double bv[4];
#pragma unroll
                for (int jb = 0; jb < 4; ++jb) {
                    const int e = (64 * w + 16 * jb + lc) * KP + 4 * ks + lk;
                    bv[jb] = F64 ? ((const double*)raw)[e] : (double)((const float*)raw)[e];
                }
#pragma unroll
                for (int jb = 0; jb < 4; ++jb) acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[jb], acc[jb], 0, 0, 0);
            }
        }
        __syncthreads();   // the row stage is consumed: its memory becomes the tile of g
        // C/D: col = lane & 15 (the row of block jb), row = (lane >> 4) + 4 reg (the candidate)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            const int rl = 64 * w + 16 * jb + lc;
            const int64_t row = row0 + rl;
            const double nr = row < a.n ? a.n64[row] : 0.0, mp = ms[rl];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int l = lk + 4 * r;
                const double key = s_cn[l] - 2.0 * acc[jb][r];
                double dd = nr + key;
                dd = dd < 0.0 ? 0.0 : dd;
                double g = dd != dd ? 0.0 : (dd < mp ? dd : mp);
                if (row >= a.n || row == s_id[l]) g = 0.0;
                gs[rl * KS_GP + l] = g;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KS_L; ++j) {   // G in full lines: 2 KiB a wave and trip
            const int e = tid + 256 * j;
            a.G[row0 * KS_L + e] = gs[(e >> 4) * KS_GP + (e & 15)];
        }
        __syncthreads();
        for (int o = KS_SEG / 2; o > 0; o >>= 1) {   // the halving tree of S26, the 16 columns side by side
            for (int e = tid; e < o * KS_L; e += 256) gs[(e >> 4) * KS_GP + (e & 15)] += gs[((e >> 4) + o) * KS_GP + (e & 15)];
            __syncthreads();
        }
        if (tid < KS_L) a.P[seg * KS_L + tid] = gs[tid];
    }
}

struct KseedPickArgs {
    const double* G;
    const double* P;
    double* T;              // [segments][16] the prefixes of this step
    int32_t* cand;
    int32_t* state;
    unsigned char* mark;    // [n] 1: chosen
    const double* U;        // [(k - 1) L]
    int64_t* ids;           // [k]
    double* phi;            // [k]
    int64_t* candrec;       // [(k - 1) L]
    int32_t* chosen;        // [k - 1]
    int64_t n, segs;
    int t, k, L;
};

__global__ __launch_bounds__(256) void kseed_pick_kernel(KseedPickArgs a) {
    __shared__ double pbuf[2][KS_PC * KS_L];
    __shared__ double col[4][KS_SEG];
    __shared__ double s_t[KS_L];
    __shared__ int64_t s_seg[KS_L];
    __shared__ double s_phi;
    __shared__ int s_l;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (a.state[KS_DEGEN]) {   // (raised by a pick launch: t >= 1) the smallest id not yet chosen; fewer than k <= n are marked
        if (tid == 0) {
            int64_t pos = a.state[KS_CURSOR];
            while (pos < a.n - 1 && a.mark[pos]) ++pos;
            a.mark[pos] = 1;
            a.ids[a.t] = pos;
            a.phi[a.t] = 0.0;
            a.chosen[a.t - 1] = -1;
            a.state[KS_CURSOR] = (int32_t)(pos + 1);
            a.state[KS_FILLED] += 1;
        }
        if (tid < a.L) a.candrec[(int64_t)(a.t - 1) * a.L + tid] = -1;
        return;
    }
    const int Lt = a.t == 0 ? 1 : a.L;
    // the 16 prefixes side by side, serial in s: lanes 0 .. 15 of wave 0 add chunk c out of LDS while waves 1 .. 3 fetch chunk c + 1
    // (full lines, many loads in flight: the serial chain never waits for memory)
    auto fetch = [&](int64_t c, int e0, int step) {
        double* dst = pbuf[c & 1];
        for (int e = e0; e < KS_PC * KS_L; e += step) {
            const int64_t s = c * KS_PC + (e >> 4);
            dst[e] = s < a.segs ? a.P[s * KS_L + (e & 15)] : 0.0;
        }
    };
    const int64_t chunks = (a.segs + KS_PC - 1) / KS_PC;
    const int l = lane & 15;
    double T = 0.0;
    fetch(0, tid, 256);
    __syncthreads();
    for (int64_t c = 0; c < chunks; ++c) {
        if (w != 0) {
            if (c + 1 < chunks) fetch(c + 1, tid - 64, 192);
        } else if (lane < KS_L) {
            const double* src = pbuf[c & 1];
            const int m = (int)min((int64_t)KS_PC, a.segs - c * KS_PC);
#pragma unroll 8
            for (int j = 0; j < m; ++j) {
                T = T + src[j * KS_L + l];
                a.T[(c * KS_PC + j) * KS_L + l] = T;
            }
        }
        __syncthreads();
    }
    if (w == 0) {
        double best = l < Lt ? T : key_traits<double>::inf();
        int bl = l;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            const double ok = __shfl_xor(best, o, 64);
            const int ol = __shfl_xor(bl, o, 64);
            if (ok < best || (ok == best && ol < bl)) {
                best = ok;
                bl = ol;
            }
        }
        if (bl >= Lt) bl = 0;   // (no comparable potential)
        const int32_t mine = lane < KS_L ? a.cand[lane] : -1;
        const int32_t id = __shfl(mine, bl, 64);
        if (lane == 0) {
            s_l = bl;
            s_phi = best;
            a.state[KS_LSTAR] = bl;
            a.ids[a.t] = id;
            a.phi[a.t] = best;
            if (id >= 0 && id < a.n) a.mark[id] = 1;
            if (a.t > 0) a.chosen[a.t - 1] = bl;
            if (!(best > 0.0)) a.state[KS_DEGEN] = 1;
        }
        if (a.t > 0 && lane < a.L) a.candrec[(int64_t)(a.t - 1) * a.L + lane] = mine;
    }
    __syncthreads();   // (also: wave 0's prefixes are visible to the block)
    const int ls = s_l;
    const double Phi = s_phi;
    if (a.t + 1 >= a.k || !(Phi > 0.0)) return;
    // the candidates of step t + 1 from the m this pick committed, G[.][l*]
    if (tid < a.L) {
        const double tt = a.U[(int64_t)a.t * a.L + tid] * Phi;
        int64_t lo = 0, hi = a.segs;   // the first s with T[s] > tt (T never falls)
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.T[mid * KS_L + ls] > tt) hi = mid;
            else lo = mid + 1;
        }
        if (lo == a.segs) {   // none: the last segment with a positive sum
            lo = a.segs - 1;
            while (lo > 0 && !(a.P[lo * KS_L + ls] > 0.0)) --lo;
        }
        s_seg[tid] = lo;
        s_t[tid] = tt;
    }
    __syncthreads();
    for (int l = w; l < a.L; l += 4) {
        const int64_t s = s_seg[l];
#pragma unroll
        for (int j = 0; j < 4; ++j) col[w][lane + 64 * j] = a.G[(s * KS_SEG + lane + 64 * j) * KS_L + ls];
        AS_LDS_FENCE();
        if (lane == 0) {
            const double tt = s_t[l];
            double r = s > 0 ? a.T[(s - 1) * KS_L + ls] : 0.0;
            int pick = -1, last = -1;
            for (int j = 0; j < KS_SEG && pick < 0; ++j) {
                const double m = col[w][j];
                r = r + m;
                if (m > 0.0) {
                    last = j;
                    if (r > tt) pick = j;
                }
            }
            if (pick < 0) pick = last;
            a.cand[l] = pick < 0 ? -1 : (int32_t)(s * KS_SEG + pick);
        }
        AS_LDS_FENCE();
    }
    if (tid >= a.L && tid < KS_L) a.cand[tid] = -1;
}

// the words of a call: nothing chosen, candidate 0 = `first`
__global__ __launch_bounds__(256) void kseed_init_kernel(unsigned char* mark, int64_t n, int32_t* cand, int32_t* state, int32_t first) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) mark[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x < KS_L) cand[threadIdx.x] = threadIdx.x == 0 ? first : -1;
    if (blockIdx.x == 0 && threadIdx.x < KS_WORDS) state[threadIdx.x] = 0;
}

// ------------------------------------------------------------------ host side
std::atomic<int> g_kseed_grid_cap{0};

// one timed launch under "kmeans_timing": events around it, added to *us (timing waits for it)
struct KseedTimer {
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

as_status kseed_run(const as_space* sp, const KseedCall& c, int64_t* counts) {
    KmeansWork* w;
    AS_TRY(kmeans_work_get(sp, &w));
    KseedWork& b = w->seed;
    const int64_t n = sp->n, segs = (n + KS_SEG - 1) / KS_SEG, k = c.k, nu = (k - 1) * c.L;
    AS_TRY(reserve_or_err(b.G, segs * KS_SEG * KS_L, "kmeans_seed candidate distances"));
    AS_TRY(reserve_or_err(b.P, segs * KS_L, "kmeans_seed segment sums"));
    AS_TRY(reserve_or_err(b.T, segs * KS_L, "kmeans_seed prefixes"));
    AS_TRY(reserve_or_err(b.U, std::max<int64_t>(nu, 1), "kmeans_seed uniforms"));
    AS_TRY(reserve_or_err(b.phi, k, "kmeans_seed potentials"));
    AS_TRY(reserve_or_err(b.ids, k, "kmeans_seed ids"));
    AS_TRY(reserve_or_err(b.candrec, std::max<int64_t>(nu, 1), "kmeans_seed candidate record"));
    AS_TRY(reserve_or_err(b.chosen, k, "kmeans_seed choices"));
    AS_TRY(reserve_or_err(b.words, KS_L + KS_WORDS, "kmeans_seed words"));
    AS_TRY(reserve_or_err(b.mark, n, "kmeans_seed marks"));
    int32_t* cand = b.words;
    int32_t* state = cand + KS_L;
    const KseedTimer tm{w, kmeans_timing_on()};
    for (double& v : b.us) v = 0.0;
    if (nu) AS_HIP(hipMemcpyAsync((double*)b.U, c.uniforms, sizeof(double) * (size_t)nu, hipMemcpyHostToDevice, w->stream));
    hipLaunchKernelGGL(kseed_init_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, w->stream,
                       (unsigned char*)b.mark, n, cand, state, (int32_t)c.first);
    KseedDistArgs da;
    da.x32 = sp->x32; da.x64 = sp->x64; da.n64 = sp->n64; da.cand = cand; da.state = state; da.G = b.G; da.P = b.P;
    da.n = n; da.d = sp->d; da.dp = sp->dp;
    KseedPickArgs pa;
    pa.G = b.G; pa.P = b.P; pa.T = b.T; pa.cand = cand; pa.state = state; pa.mark = b.mark; pa.U = b.U; pa.ids = b.ids; pa.phi = b.phi;
    pa.candrec = b.candrec; pa.chosen = b.chosen; pa.n = n; pa.segs = segs; pa.k = (int)k; pa.L = c.L;
    const int64_t cap = g_kseed_grid_cap.load(std::memory_order_relaxed);
    const unsigned grid = (unsigned)(cap > 0 ? std::min(segs, cap) : segs);
    for (int64_t t = 0; t < k; ++t) {
        da.first = t == 0 ? 1 : 0;
        pa.t = (int)t;
        AS_TRY(tm.begin());
        if (sp->x64) hipLaunchKernelGGL(kseed_dist_kernel<true>, dim3(grid), dim3(256), 0, w->stream, da);
        else hipLaunchKernelGGL(kseed_dist_kernel<false>, dim3(grid), dim3(256), 0, w->stream, da);
        AS_TRY(tm.end(&b.us[0]));
        AS_TRY(tm.begin());
        hipLaunchKernelGGL(kseed_pick_kernel, dim3(1), dim3(256), 0, w->stream, pa);
        AS_TRY(tm.end(&b.us[1]));
    }
    AS_HIP(hipGetLastError());
    counts[0] += k - 1;
    counts[1] += k;
    counts[2] += k;
    int32_t words[KS_WORDS] = {0, 0, 0, 0};
    AS_HIP(hipMemcpyAsync(c.out_ids, (const int64_t*)b.ids, sizeof(int64_t) * (size_t)k, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipMemcpyAsync(c.out_phi, (const double*)b.phi, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, w->stream));
    if (nu) {
        AS_HIP(hipMemcpyAsync(c.out_cand, (const int64_t*)b.candrec, sizeof(int64_t) * (size_t)nu, hipMemcpyDeviceToHost, w->stream));
        AS_HIP(hipMemcpyAsync(c.out_chosen, (const int32_t*)b.chosen, sizeof(int32_t) * (size_t)(k - 1), hipMemcpyDeviceToHost, w->stream));
    }
    AS_HIP(hipMemcpyAsync(words, (const int32_t*)state, sizeof(words), hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[3] += 1;
    c.out_info[0] = words[KS_FILLED];
    b.us[2] = (double)(k - 1);
    return AS_OK;
}

}  // namespace

void set_kmeans_seed_grid_cap(int v) { g_kseed_grid_cap.store(v > 0 ? v : 0, std::memory_order_relaxed); }

double kmeans_seed_kernel_us(const KmeansWork* w, int part) { return w && part >= 0 && part < 3 ? w->seed.us[part] : 0.0; }

as_status kmeans_seed(const as_space* sp, const KseedCall& c, int64_t* counts) {
    const as_status s = kseed_run(sp, c, counts);
    // (a failed run leaves nothing on the stream when the caller releases the lock)
    if (s != AS_OK && sp->kmeans_ws && sp->kmeans_ws->stream) (void)hipStreamSynchronize(sp->kmeans_ws->stream);
    return s;
}

}  // namespace as
