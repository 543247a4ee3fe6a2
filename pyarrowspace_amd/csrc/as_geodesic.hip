// Graph shortest paths over the item graph (section 5.27): d[v] = the minimum, over the seeds s of a
// column and the paths s = p0 .. pm = v, of fl(.. fl(fl(off_s + w1) + w2) .. + wm), +inf where no path leads.  The weight of the
// undirected edge {u, v} is S23's (the smaller of its two stored dists, a NaN ignored, -0.0 as +0.0): the images fr_weights_kernel
// writes, kept in the workspace across calls under the graph's serial.  An edge whose weight is a NaN or negative is never crossed.
// For w >= 0, x -> fl(x + w) is monotone and never below x, so the least fixed point of d[v] = min(d[v], fl(d[u] + w(u, v))) from
// d[seed] = offset is unique: it is what a Dijkstra with the same add returns, bit for bit, whatever the order of the relaxations.
// Two routes, by the columns of a chunk (the diffusion forms' widths and "diffuse_mib" budget):
//   C = 1   PUSH over a frontier.  d[n] holds the fp64 bit patterns (for non-negative doubles unsigned order is numeric order):
//           one 64-bit atomicMin relaxes an edge.  A sub-wave of W lanes ("geodesic_row_lanes") owns a frontier row: it reads d[u]
//           once, strides the entries, forms fl(d[u] + w), drops candidates above the cutoff, reads d[v] plainly and issues the
//           atomic only where the candidate is smaller (a stale read is a larger one: it can only cost an atomic).  An item whose
//           word went down enters the next near list once per round (stamp[v] exchanged with the round's number) if its new d is
//           <= T, else the far list once (a flag) -- both by one atomic on the list's tail per wave and ballot ranks.  When the near
//           list runs empty T advances by "geodesic_delta" and a filter launch moves the far items with d <= T to the near list and
//           drops those the near rounds have served since (d <= the T they ran under).  While the near list holds at most R rows
//           ("geodesic_lds_rows") ONE block keeps it in two LDS lists and runs round after round with barriers between, until
//           the list empties or outgrows R; then it spills to the global list and the grid-wide kernel goes on.  The host reads
//           the list lengths once per launch through pinned memory.
//   C = 16, 64   PULL, lanes own columns, no atomics.  d is one [n][C] block of doubles relaxed in place: a wave owns one row at
//           C = 64 and four at C = 16, w[e] and indices[e] are uniform over a row's lanes, d[j][0 .. C) is one contiguous segment,
//           a lane keeps four independent minima over fl(d[j][c] + w).  Only the owner writes row i.  stamp[j] is the last round in
//           which a column of row j went down: in round r row i first streams its neighbours' stamps and relaxes only if one is
//           >= r - 1.  A change of j in round r after i looked is seen by i in round r + 1 through stamp[j] = r; a round without a
//           change read only values nobody changed in it, so it is the fixed point: the host stops after it (one flag word).
// Nothing depends on the grid, on W, on delta, on R, on the chunk width or on the order of the atomics: every word only ever
// decreases, over a finite set of values, towards the one fixed point.
// Entry points: as_api.hip (as_geodesic_seeds, as_search_geodesic, as_search_geodesic_batch, as_geodesic_counters,
// as_geodesic_kernel_us).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "as_diffuse.hpp"

namespace as {

namespace {

constexpr unsigned long long GD_INF = 0x7ff0000000000000ull;   // the bits of +inf: above every finite non-negative double's
constexpr unsigned long long GD_NONE = ~0ull;
constexpr int GD_LDS_THREADS = 1024;       // threads of the one-block kernel: sixteen waves hide the latency of one CU's gathers
constexpr int GD_LDS_ROWS_DEFAULT = 2048;  // a choice, not a measurement (section 5.27)
constexpr int GD_LDS_ROWS_MAX = 4096;      // two lists of ids: 32 KiB of LDS

// what a launch leaves on the device and the host reads: 80 bytes at the start of their allocation
struct GdStat {
    unsigned long long nlen[2];   // the tails of the two near lists
    unsigned long long flen[2];   // ... and of the two far lists
    unsigned long long fmin[2];   // the smallest d (bits) a filter kept in the far list of that index, GD_NONE
    unsigned long long relax;     // words lowered
    unsigned long long rounds;    // rounds the last one-block launch ran
    unsigned long long flag;      // pull: the number of the last round in which a row went down
    unsigned long long active;    // pull: CSR entries of the rows that relaxed (the others read 8 bytes per entry and skipped)
};
constexpr int GD_STAT_WORDS = sizeof(GdStat) / 8;

struct GdArgs {
    const int64_t* indptr;    // [n + 1]
    const int32_t* indices;   // [nnz]
    const unsigned long long* wkey;   // [nnz]
    unsigned long long* d;    // [n] bit patterns
    int32_t* stamp;           // [n] the last round in which the item was put on a near list
    int32_t* farflag;         // [n] 1: the item is on the far list
    int32_t* near[2];         // [n] each
    int32_t* far[2];          // [n] each
    GdStat* stat;
    int64_t n;
    double cutoff;            // candidates above it are never stored (+inf: none)
    double T, Tdone;          // near: d <= T; the filter drops d <= Tdone
    int64_t len;              // entries of the list the launch consumes (the host read it)
    int32_t round;            // the number of the launch's (first) round, from 1
    int cur, fcur;            // the near list consumed (appends go to the other); the far list appended to
    int lds_rows;             // R
};

__device__ __forceinline__ double gd_dbl(unsigned long long b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ unsigned long long gd_word(double x) { return (unsigned long long)__double_as_longlong(x); }
// the weight behind an image; false: a NaN or a negative number, never crossed
__device__ __forceinline__ bool gd_weight(unsigned long long key, double* w) {
    if (!(key & FR_SIGN) || key == FR_NAN) return false;
    *w = gd_dbl(forest_bits(key));
    return true;
}
// the same as a number the pull route can add without a branch: +inf never lowers a minimum
__device__ __forceinline__ double gd_weight_or_inf(unsigned long long key) {
    double w;
    return gd_weight(key, &w) ? w : gd_dbl(GD_INF);
}

// The place of a lane's entry in a list, wave-aggregated (range search's compaction): EVERY lane of the wave calls it; one atomic on
// the tail per wave, the lanes that want a place take their ballot rank.  -1: no place wanted.
template <typename T>
__device__ __forceinline__ int64_t gd_slot(bool want, T* tail) {
    const unsigned long long mask = __ballot(want);
    if (!mask) return -1;
    const int lane = lane_id(), leader = __ffsll((long long)mask) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = (unsigned long long)atomicAdd(tail, (T)__popcll(mask));
    base = __shfl(base, leader);
    return want ? (int64_t)(base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1))) : -1;
}

__device__ __forceinline__ void gd_add_relaxed(unsigned long long relaxed, GdStat* stat) {
    for (int o = 32; o > 0; o >>= 1) relaxed += __shfl_down(relaxed, o);
    if (lane_id() == 0 && relaxed) atomicAdd(&stat->relax, relaxed);
}

// One frontier row by a sub-wave of W lanes (live false: the sub-wave has no row, and only keeps the wave's ballots whole).  The
// loop runs while ANY lane of the wave has an entry left, so every lane meets every ballot.  LDS: the next near list is lnext
// (lds_rows places, tail *ltail), what does not fit goes to gnear behind; else gnear under its tail in stat.
template <int W, bool LDS>
__device__ __forceinline__ void gd_relax_row(const GdArgs& a, int32_t u, bool live, int lane, int32_t round, int32_t* lnext,
                                             unsigned int* ltail, int32_t* gnear, unsigned long long* gtail, unsigned long long& relaxed) {
    int64_t e = 0, e1 = 0;
    double du = 0.0;
    if (live) {
        e = a.indptr[u] + lane;
        e1 = a.indptr[u + 1];
        // (past this CU's first-level cache: the one-block kernel reads what its own earlier rounds lowered)
        du = gd_dbl(__hip_atomic_load(&a.d[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    while (__ballot(e < e1)) {
        bool tonear = false, tofar = false;
        int32_t v = 0;
        if (e < e1) {
            v = a.indices[e];
            double w;
            if (gd_weight(a.wkey[e], &w)) {
                const double c = du + w;
                const unsigned long long cw = gd_word(c);
                if (c <= a.cutoff && cw < a.d[v] && cw < atomicMin(&a.d[v], cw)) {
                    ++relaxed;
                    if (c <= a.T) tonear = atomicExch(&a.stamp[v], round) != round;
                    else tofar = atomicExch(&a.farflag[v], 1) == 0;
                }
            }
        }
        if (LDS) {
            const int64_t at = gd_slot(tonear, ltail);
            if (at >= 0) {
                if (at < a.lds_rows) lnext[at] = v;
                else gnear[at - a.lds_rows] = v;
            }
        } else {
            const int64_t at = gd_slot(tonear, gtail);
            if (at >= 0) gnear[at] = v;
        }
        const int64_t fat = gd_slot(tofar, &a.stat->flen[a.fcur]);
        if (fat >= 0) a.far[a.fcur][fat] = v;
        e += W;
    }
}

// d = +inf, stamp = 0, no far flag; the words of GdStat
__global__ __launch_bounds__(DIF_THREADS) void gd_init_kernel(GdArgs a) {
    for (int64_t x = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; x < a.n; x += (int64_t)gridDim.x * DIF_THREADS) {
        a.d[x] = GD_INF;
        a.stamp[x] = 0;
        a.farflag[x] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        GdStat* s = a.stat;
        s->nlen[0] = s->nlen[1] = s->flen[0] = s->flen[1] = 0;
        s->fmin[0] = s->fmin[1] = GD_NONE;
        s->relax = s->rounds = s->flag = s->active = 0;
    }
}

// The seeds of the column, by one block: d[item] = min(d[item], offset) unless the offset lies above the cutoff; near list 0 or
// far list 0.  (The ids of a column are distinct: every seed is appended once.)
__global__ __launch_bounds__(DIF_THREADS) void gd_seed_kernel(GdArgs a, const int32_t* __restrict__ item, const double* __restrict__ val, int64_t ns) {
    for (int64_t t0 = 0; t0 < ns; t0 += DIF_THREADS) {
        const int64_t t = t0 + threadIdx.x;
        bool tonear = false, tofar = false;
        int32_t v = 0;
        if (t < ns) {
            v = item[t];
            double off = val[t];
            if (off == 0.0) off = 0.0;
            if (off <= a.cutoff) {
                atomicMin(&a.d[v], gd_word(off));
                tonear = off <= a.T;
                tofar = !tonear;
                if (tofar) a.farflag[v] = 1;
            }
        }
        const int64_t at = gd_slot(tonear, &a.stat->nlen[0]);
        if (at >= 0) a.near[0][at] = v;
        const int64_t fat = gd_slot(tofar, &a.stat->flen[0]);
        if (fat >= 0) a.far[0][fat] = v;
    }
}

// One grid-wide round: the rows of near[cur], DIF_THREADS / W of them per block and trip; appends to near[cur ^ 1], whose tail the
// round before last cleared.
template <int W>
__global__ __launch_bounds__(DIF_THREADS) void gd_relax_kernel(GdArgs a) {
    constexpr int ROWS = DIF_THREADS / W;
    const int sub = threadIdx.x / W, lane = threadIdx.x % W, nxt = a.cur ^ 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.stat->nlen[a.cur] = 0;   // consumed: its length came with the arguments
    unsigned long long relaxed = 0;
    const int64_t trips = (a.len + ROWS - 1) / ROWS;
    for (int64_t g = blockIdx.x; g < trips; g += gridDim.x) {
        const int64_t t = g * ROWS + sub;
        const bool live = t < a.len;
        gd_relax_row<W, false>(a, live ? a.near[a.cur][t] : 0, live, lane, a.round, nullptr, nullptr, a.near[nxt], &a.stat->nlen[nxt], relaxed);
    }
    gd_add_relaxed(relaxed, a.stat);
}

// The rounds of a small frontier by ONE block: near[cur] (len <= R) into LDS, then round after round between two LDS lists against
// the global d, until the next list is empty or has outgrown R; that list goes to near[cur ^ 1] (what did not fit is there
// already, the R ids of the LDS list behind it).  A word only ever decreases over a finite set of values: the loop ends.
template <int W>
__global__ __launch_bounds__(GD_LDS_THREADS) void gd_lds_kernel(GdArgs a) {
    extern __shared__ int32_t gd_lists[];
    __shared__ unsigned int s_tail;
    constexpr int ROWS = GD_LDS_THREADS / W;
    const int tid = threadIdx.x, sub = tid / W, lane = tid % W, nxt = a.cur ^ 1, R = a.lds_rows;
    int32_t* A = gd_lists;
    int32_t* B = gd_lists + R;
    int len = (int)a.len;
    for (int t = tid; t < len; t += GD_LDS_THREADS) A[t] = a.near[a.cur][t];
    if (tid == 0) s_tail = 0;
    __syncthreads();
    unsigned long long relaxed = 0;
    int32_t round = a.round;
    for (;;) {
        for (int t0 = 0; t0 < len; t0 += ROWS) {
            const int t = t0 + sub;
            const bool live = t < len;
            gd_relax_row<W, true>(a, live ? A[t] : 0, live, lane, round, B, &s_tail, a.near[nxt], nullptr, relaxed);
        }
        __syncthreads();
        const unsigned int tail = s_tail;
        __syncthreads();   // every thread has read the tail before it is cleared
        if (tail == 0 || tail > (unsigned int)R) {
            if (tail > 0)
                for (int t = tid; t < R; t += GD_LDS_THREADS) a.near[nxt][tail - (unsigned int)R + t] = B[t];
            if (tid == 0) {
                a.stat->nlen[nxt] = tail;
                a.stat->nlen[a.cur] = 0;
                a.stat->rounds = (unsigned long long)(round - a.round + 1);
            }
            break;
        }
        if (tid == 0) s_tail = 0;
        int32_t* const swap = A;
        A = B;
        B = swap;
        len = (int)tail;
        ++round;
        __syncthreads();
    }
    gd_add_relaxed(relaxed, a.stat);
}

// The bucket's advance: far[fcur] (len entries) -> near[cur] where Tdone < d <= T, far[fcur ^ 1] where d > T (with the smallest such
// d in fmin[fcur ^ 1]); an entry with d <= Tdone went to a near list when it got there and is dropped.  Clears the tail and the
// minimum of the list it consumed, for the filter after the next.
__global__ __launch_bounds__(DIF_THREADS) void gd_filter_kernel(GdArgs a) {
    const int fnxt = a.fcur ^ 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.stat->flen[a.fcur] = 0;
        a.stat->fmin[a.fcur] = GD_NONE;
    }
    unsigned long long least = GD_NONE;
    const int64_t trips = (a.len + DIF_THREADS - 1) / DIF_THREADS;
    for (int64_t g = blockIdx.x; g < trips; g += gridDim.x) {
        const int64_t t = g * DIF_THREADS + threadIdx.x;
        const bool live = t < a.len;
        const int32_t v = live ? a.far[a.fcur][t] : 0;
        const unsigned long long dw = live ? a.d[v] : 0;
        const double dv = gd_dbl(dw);
        const bool keep = live && dv > a.T, move = live && !keep && dv > a.Tdone;
        if (live && !keep) a.farflag[v] = 0;
        if (keep && dw < least) least = dw;
        const int64_t at = gd_slot(move, &a.stat->nlen[a.cur]);
        if (at >= 0) a.near[a.cur][at] = v;
        const int64_t fat = gd_slot(keep, &a.stat->flen[fnxt]);
        if (fat >= 0) a.far[fnxt][fat] = v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_down(least, o);
        least = other < least ? other : least;
    }
    if (lane_id() == 0 && least != GD_NONE) atomicMin(&a.stat->fmin[fnxt], least);
}

// ---- the pull route
struct GpArgs {
    const int64_t* indptr;
    const int32_t* indices;
    const unsigned long long* wkey;
    double* d;         // [n][C]
    int32_t* stamp;    // [n] the last round in which a column of the row went down; a seed's row: 0; else -2
    GdStat* stat;
    int64_t n;
    double cutoff;
    int32_t round;
};

__global__ __launch_bounds__(DIF_THREADS) void gp_init_kernel(GpArgs a, int C) {
    const double inf = gd_dbl(GD_INF);
    for (int64_t x = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; x < a.n * C; x += (int64_t)gridDim.x * DIF_THREADS) {
        a.d[x] = inf;
        if (x < a.n) a.stamp[x] = -2;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.stat->relax = a.stat->flag = a.stat->active = 0;
}

// the seed table of the chunk (diffuse_seed_table: distinct (item, column) pairs) by min onto the +inf fill
__global__ __launch_bounds__(DIF_THREADS) void gp_seed_kernel(GpArgs a, int C, const int32_t* __restrict__ item, const int32_t* __restrict__ col,
                                                              const double* __restrict__ val, int64_t ns) {
    for (int64_t t = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; t < ns; t += (int64_t)gridDim.x * DIF_THREADS) {
        double off = val[t];
        if (off == 0.0) off = 0.0;
        if (!(off <= a.cutoff)) continue;
        double* cell = a.d + (int64_t)item[t] * C + col[t];
        if (off < *cell) *cell = off;
        a.stamp[item[t]] = 0;
    }
}

template <int CT>
__global__ __launch_bounds__(DIF_THREADS) void gp_pull_kernel(GpArgs a) {
    constexpr int RPW = 64 / CT;
    __shared__ int s_seen;
    if (threadIdx.x == 0) s_seen = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, c = lane % CT, sub = lane / CT;
    const int64_t waves = (int64_t)gridDim.x * (DIF_THREADS / 64);
    const double* f = a.d + c;   // (no __restrict__: the rows read are rows other waves write)
    bool seen = false;
    unsigned long long relaxed = 0, entries = 0;
    for (int64_t r0 = ((int64_t)blockIdx.x * (DIF_THREADS / 64) + (threadIdx.x >> 6)) * RPW; r0 < a.n; r0 += waves * RPW) {
        const int64_t row = r0 + sub;
        if (row >= a.n) continue;   // (the CT lanes of a row leave together: the cross-lane moves below stay inside a row's lanes)
        const int64_t rs = a.indptr[row], re = a.indptr[row + 1];
        int active = 0;   // 8 bytes per entry: the column and its stamp
        for (int64_t e = rs + c; e < re; e += CT) active |= a.stamp[a.indices[e]] >= a.round - 1;
        for (int o = CT / 2; o > 0; o >>= 1) active |= __shfl_xor(active, o, CT);
        if (!active) continue;
        if (c == 0) entries += (unsigned long long)(re - rs);
        const double own = f[row * CT];
        double m0 = own, m1 = own, m2 = own, m3 = own;
        int64_t e = rs;
        for (; e + 4 <= re; e += 4) {
            const double w0 = gd_weight_or_inf(a.wkey[e]), w1 = gd_weight_or_inf(a.wkey[e + 1]);
            const double w2 = gd_weight_or_inf(a.wkey[e + 2]), w3 = gd_weight_or_inf(a.wkey[e + 3]);
            const double v0 = f[(int64_t)a.indices[e] * CT] + w0, v1 = f[(int64_t)a.indices[e + 1] * CT] + w1;
            const double v2 = f[(int64_t)a.indices[e + 2] * CT] + w2, v3 = f[(int64_t)a.indices[e + 3] * CT] + w3;
            m0 = v0 < m0 ? v0 : m0;
            m1 = v1 < m1 ? v1 : m1;
            m2 = v2 < m2 ? v2 : m2;
            m3 = v3 < m3 ? v3 : m3;
        }
        for (; e < re; ++e) {
            const double v = f[(int64_t)a.indices[e] * CT] + gd_weight_or_inf(a.wkey[e]);
            m0 = v < m0 ? v : m0;
        }
        m0 = m1 < m0 ? m1 : m0;
        m2 = m3 < m2 ? m3 : m2;
        m0 = m2 < m0 ? m2 : m0;
        int down = m0 < own && m0 <= a.cutoff;   // (the smallest candidate passes the cutoff, or none does)
        if (down) {
            a.d[row * CT + c] = m0;
            ++relaxed;
        }
        for (int o = CT / 2; o > 0; o >>= 1) down |= __shfl_xor(down, o, CT);
        if (down) {
            if (c == 0) a.stamp[row] = a.round;
            seen = true;
        }
    }
    if (seen) s_seen = 1;   // (every writer stores the same value)
    gd_add_relaxed(relaxed, a.stat);
    for (int o = 32; o > 0; o >>= 1) entries += __shfl_down(entries, o);
    if (lane_id() == 0 && entries) atomicAdd(&a.stat->active, entries);
    __syncthreads();
    if (threadIdx.x == 0 && s_seen) atomicMax(&a.stat->flag, (unsigned long long)a.round);
}

// x <- -x over the block: what the selection ranks (d ascending is -d descending; +inf becomes -inf)
__global__ __launch_bounds__(DIF_THREADS) void gd_negate_kernel(double* d, int64_t count) {
    for (int64_t x = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; x < count; x += (int64_t)gridDim.x * DIF_THREADS) d[x] = -d[x];
}

// ------------------------------------------------------------------ host side
std::atomic<int> g_row_lanes{16};   // a choice (the forest's fastest): 8, 16 and 32 measured alike on the one graph tried (section 5.27)
std::atomic<int> g_lds_rows{GD_LDS_ROWS_DEFAULT};
std::atomic<double> g_delta{0.0};

unsigned gd_grid(const DiffuseWork* w, int64_t blocks) { return diffuse_grid(std::min<int64_t>(blocks, (int64_t)w->cus * DIF_BLOCKS_PER_CU)); }

// one timed part: the launches between begin() and end() on the work's stream, added to *us (timing waits for them)
struct GdTimer {
    DiffuseWork* w;
    bool on;
    as_status begin() const {
        if (on) AS_HIP(hipEventRecord(w->gd_ev.e[0], w->stream));
        return AS_OK;
    }
    as_status end(double* us) const {
        if (!on) return AS_OK;
        AS_HIP(hipEventRecord(w->gd_ev.e[1], w->stream));
        AS_HIP(hipEventSynchronize(w->gd_ev.e[1]));
        float ms = 0.0f;
        AS_HIP(hipEventElapsedTime(&ms, w->gd_ev.e[0], w->gd_ev.e[1]));
        *us += (double)ms * 1e3;
        return AS_OK;
    }
};

// the words of GdStat to the pinned copy: one wait
as_status gd_read(DiffuseWork* w, int64_t* counts) {
    AS_HIP(hipGetLastError());
    AS_HIP(hipMemcpyAsync((unsigned long long*)w->gd_stat_h, (const unsigned long long*)w->gd_stat_d, sizeof(GdStat), hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[3] += 1;
    return AS_OK;
}

// the images of the graph's weights in w->fr_wkey: kept from the last call on this graph (a forest's or a shortest paths'), else one launch
as_status gd_weights(DiffuseWork* w, const as_graph* gr, const GdTimer& tm, int64_t* counts) {
    if (gr->nnz <= 0 || (w->fr_wkey_serial == gr->serial && (int64_t)w->fr_wkey.size() >= gr->nnz)) return AS_OK;
    w->fr_wkey_serial = 0;
    AS_TRY(reserve_or_err(w->fr_wkey, gr->nnz, "forest weights"));
    AS_TRY(tm.begin());
    hipLaunchKernelGGL(fr_weights_kernel, dim3(gd_grid(w, (gr->n + DIF_THREADS - 1) / DIF_THREADS)), dim3(DIF_THREADS), 0, w->stream,
                       (const int64_t*)gr->indptr, (const int32_t*)gr->indices, (const double*)gr->dist, (unsigned long long*)w->fr_wkey, gr->n);
    AS_HIP(hipGetLastError());
    AS_TRY(tm.end(&w->gd_us[0]));
    w->fr_wkey_serial = gr->serial;
    w->gd_us[6] += 1.0;
    counts[2] += 1;
    return AS_OK;
}

double gd_host_dbl(unsigned long long b) {
    double v;
    memcpy(&v, &b, sizeof(v));
    return v;
}

// a row kernel under "geodesic_row_lanes"
using GdRowKernel = void (*)(GdArgs);
void gd_launch_rows(GdRowKernel k8, GdRowKernel k16, GdRowKernel k32, int lanes, unsigned grid, unsigned threads, size_t lds, hipStream_t stream,
                    const GdArgs& a) {
    hipLaunchKernelGGL(lanes == 8 ? k8 : (lanes == 32 ? k32 : k16), dim3(grid), dim3(threads), lds, stream, a);
}

// One column by the push route: the seeds [s0, s1) of the uploaded table -> d (w->gd_d, [n] bit patterns).  *rounds: the rounds run.
as_status gd_push(DiffuseWork* w, const as_graph* gr, const DiffuseSeeds& sd, double cutoff, const GdTimer& tm, int64_t* rounds, int64_t* counts) {
    const int64_t n = gr->n;
    const int lanes = g_row_lanes.load(std::memory_order_relaxed), R = g_lds_rows.load(std::memory_order_relaxed);
    const double delta = g_delta.load(std::memory_order_relaxed), inf = std::numeric_limits<double>::infinity();
    GdStat* stat = (GdStat*)(unsigned long long*)w->gd_stat_d;
    const GdStat* host = (const GdStat*)(unsigned long long*)w->gd_stat_h;
    int32_t* ints = w->gd_ints;
    GdArgs a;
    a.indptr = gr->indptr; a.indices = gr->indices; a.wkey = w->fr_wkey; a.d = w->gd_d; a.stat = stat; a.n = n; a.cutoff = cutoff;
    a.stamp = ints; a.farflag = ints + n; a.near[0] = ints + 2 * n; a.near[1] = ints + 3 * n; a.far[0] = ints + 4 * n; a.far[1] = ints + 5 * n;
    a.T = delta > 0.0 ? delta : inf; a.Tdone = -1.0; a.len = 0; a.round = 1; a.cur = 0; a.fcur = 0; a.lds_rows = R;
    hipLaunchKernelGGL(gd_init_kernel, dim3(gd_grid(w, (n + DIF_THREADS - 1) / DIF_THREADS)), dim3(DIF_THREADS), 0, w->stream, a);
    if (sd.ns > 0) hipLaunchKernelGGL(gd_seed_kernel, dim3(1), dim3(DIF_THREADS), 0, w->stream, a, sd.item, sd.val, sd.ns);
    counts[2] += sd.ns > 0 ? 2 : 1;
    AS_TRY(gd_read(w, counts));
    int64_t nl = (int64_t)host->nlen[0], fl = (int64_t)host->flen[0];
    bool have_least = false;   // the last launch was a filter that moved nothing: fmin[fcur] is the far list's smallest d
    *rounds = 0;
    while (nl > 0 || fl > 0) {
        if (nl > n || fl > n) {
            set_err("geodesic: the device reported lists of %lld and %lld items for %lld items", (long long)nl, (long long)fl, (long long)n);
            return AS_EHIP;
        }
        if (nl == 0) {   // the bucket's advance
            double T = a.T + delta;
            if (have_least) T = std::max(T, gd_host_dbl(host->fmin[a.fcur]));   // at least the smallest item moves
            a.T = T;
            a.len = fl;
            AS_TRY(tm.begin());
            hipLaunchKernelGGL(gd_filter_kernel, dim3(gd_grid(w, (fl + DIF_THREADS - 1) / DIF_THREADS)), dim3(DIF_THREADS), 0, w->stream, a);
            AS_TRY(tm.end(&w->gd_us[3]));
            counts[2] += 1;
            a.fcur ^= 1;
            AS_TRY(gd_read(w, counts));
            nl = (int64_t)host->nlen[a.cur];
            fl = (int64_t)host->flen[a.fcur];
            have_least = nl == 0 && host->fmin[a.fcur] != GD_NONE;
            continue;
        }
        have_least = false;
        a.Tdone = a.T;
        a.len = nl;
        AS_TRY(tm.begin());
        int64_t ran = 1;
        if (R > 0 && nl <= R) {
            gd_launch_rows(gd_lds_kernel<8>, gd_lds_kernel<16>, gd_lds_kernel<32>, lanes, 1, GD_LDS_THREADS, sizeof(int32_t) * 2 * (size_t)R, w->stream, a);
            AS_TRY(tm.end(&w->gd_us[1]));
            w->gd_us[9] += 1.0;
        } else {
            const int64_t per = DIF_THREADS / lanes;
            gd_launch_rows(gd_relax_kernel<8>, gd_relax_kernel<16>, gd_relax_kernel<32>, lanes, gd_grid(w, (nl + per - 1) / per), DIF_THREADS, 0, w->stream, a);
            AS_TRY(tm.end(&w->gd_us[2]));
            w->gd_us[10] += 1.0;
        }
        counts[2] += 1;
        AS_TRY(gd_read(w, counts));
        if (R > 0 && nl <= R) ran = (int64_t)host->rounds;
        if (ran < 1 || ran > (int64_t)1 << 30) {
            set_err("geodesic: the device reported %lld rounds of one launch", (long long)ran);
            return AS_EHIP;
        }
        *rounds += ran;
        a.round += (int32_t)ran;
        a.cur ^= 1;
        nl = (int64_t)host->nlen[a.cur];
        fl = (int64_t)host->flen[a.fcur];
    }
    return AS_OK;
}

// A chunk of C = 16 or 64 columns by the pull route -> d (w->gd_d, [n][C] doubles)
as_status gd_pull(DiffuseWork* w, const as_graph* gr, const DiffuseSeeds& sd, int C, double cutoff, const GdTimer& tm, int64_t* rounds,
                  int64_t* counts) {
    const int64_t n = gr->n;
    GdStat* stat = (GdStat*)(unsigned long long*)w->gd_stat_d;
    const GdStat* host = (const GdStat*)(unsigned long long*)w->gd_stat_h;
    GpArgs a;
    a.indptr = gr->indptr; a.indices = gr->indices; a.wkey = w->fr_wkey; a.d = (double*)(unsigned long long*)w->gd_d; a.stamp = w->gd_ints;
    a.stat = stat; a.n = n; a.cutoff = cutoff; a.round = 0;
    hipLaunchKernelGGL(gp_init_kernel, dim3(gd_grid(w, (n * C + DIF_THREADS - 1) / DIF_THREADS)), dim3(DIF_THREADS), 0, w->stream, a, C);
    if (sd.ns > 0) hipLaunchKernelGGL(gp_seed_kernel, dim3(sd.grid), dim3(DIF_THREADS), 0, w->stream, a, C, sd.item, sd.col, sd.val, sd.ns);
    counts[2] += sd.ns > 0 ? 2 : 1;
    const int64_t per_block = (int64_t)(DIF_THREADS / 64) * (64 / C);
    const unsigned grid = gd_grid(w, (n + per_block - 1) / per_block);
    *rounds = 0;
    for (;;) {
        a.round = (int32_t)++*rounds;
        AS_TRY(tm.begin());
        if (C == 16) hipLaunchKernelGGL(gp_pull_kernel<16>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
        else hipLaunchKernelGGL(gp_pull_kernel<64>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
        AS_TRY(tm.end(&w->gd_us[4]));
        counts[2] += 1;
        w->gd_us[8] += (double)gr->nnz;
        AS_TRY(gd_read(w, counts));
        if (host->flag != (unsigned long long)*rounds) {   // no row went down in this round
            w->gd_us[11] += (double)host->active;
            break;
        }
        if (*rounds >= std::numeric_limits<int32_t>::max() - 2) {
            set_err("geodesic: no fixed point within %lld rounds", (long long)*rounds);
            return AS_EHIP;
        }
    }
    return AS_OK;
}

as_status gd_run(const as_space* sp, const as_graph* gr, const GeodesicCall& c, int64_t* counts) {
    const int64_t n = gr->n;
    DiffuseFrame fr;
    AS_TRY(diffuse_frame(sp, gr, c.dc, &fr));
    if (c.chunks) *c.chunks = 0;
    if (c.relaxations) *c.relaxations = 0;
    if (!fr.w) return AS_OK;
    DiffuseWork* w = fr.w;
    const GdTimer tm{w, diffuse_timing()};
    for (double& v : w->gd_us) v = 0.0;
    if (tm.on && !w->gd_ev.e[0]) AS_HIP(w->gd_ev.create());
    AS_TRY(reserve_or_err(w->gd_stat_d, GD_STAT_WORDS, "geodesic words"));
    AS_TRY(reserve_or_err(w->gd_stat_h, GD_STAT_WORDS, "geodesic pinned words"));
    AS_TRY(reserve_or_err(w->gd_ints, 6 * n, "geodesic lists"));
    AS_TRY(gd_weights(w, gr, tm, counts));
    const GdStat* host = (const GdStat*)(unsigned long long*)w->gd_stat_h;
    const int cols_cap = diffuse_cols_cap();
    const int64_t budget = diffuse_budget(), nq = (int64_t)fr.q.size();
    for (int64_t i0 = 0; i0 < nq;) {
        const int C = diffuse_chunk_cols(nq - i0, n, cols_cap, budget, 1);
        const int64_t nc = std::min<int64_t>(C, nq - i0);
        AS_TRY(reserve_or_err(w->gd_d, n * C, "geodesic distances"));
        DiffuseSeeds sd;
        AS_TRY(diffuse_seed_table(fr, c.dc, i0, nc, &sd));
        int64_t rounds = 0;
        AS_TRY(C == 1 ? gd_push(w, gr, sd, c.cutoff, tm, &rounds, counts) : gd_pull(w, gr, sd, C, c.cutoff, tm, &rounds, counts));
        counts[0] += 1;
        counts[1] += rounds;
        w->gd_us[7] += (double)rounds;
        if (c.rounds) c.rounds[*c.chunks] = rounds;
        if (c.chunks) *c.chunks += 1;
        if (c.relaxations) *c.relaxations += (int64_t)host->relax;
        double* d = (double*)(unsigned long long*)w->gd_d;
        const auto t0 = std::chrono::steady_clock::now();
        if (fr.select) {
            hipLaunchKernelGGL(gd_negate_kernel, dim3(gd_grid(w, (n * C + DIF_THREADS - 1) / DIF_THREADS)), dim3(DIF_THREADS), 0, w->stream, d, n * C);
            AS_HIP(hipGetLastError());
            counts[2] += 1;
        }
        double unused = 0.0;
        AS_TRY(diffuse_emit(fr, c.dc, i0, nc, C, d, false, &unused));
        counts[3] += 1;
        w->gd_us[5] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        i0 += nc;
    }
    return AS_OK;
}

}  // namespace

void set_geodesic_row_lanes(int v) { g_row_lanes.store(v == 8 || v == 32 ? v : 16, std::memory_order_relaxed); }
void set_geodesic_lds_rows(int v) { g_lds_rows.store(v < 0 ? GD_LDS_ROWS_DEFAULT : std::min(v, GD_LDS_ROWS_MAX), std::memory_order_relaxed); }
void set_geodesic_delta(double v) { g_delta.store(v > 0.0 ? v : 0.0, std::memory_order_relaxed); }   // (a NaN: one bucket)

double geodesic_kernel_us(const DiffuseWork* w, int part) { return w && part >= 0 && part < 12 ? w->gd_us[part] : 0.0; }

// (a failed run leaves nothing on the stream when the caller releases the lock)
as_status geodesic_run(const as_space* sp, const as_graph* gr, const GeodesicCall& c, int64_t* counts) {
    as_status s;
    try {
        s = gd_run(sp, gr, c, counts);
    } catch (const std::bad_alloc&) {
        set_err("geodesic: out of host memory");
        s = AS_ENOMEM;
    }
    if (s != AS_OK && sp->diffuse_ws) (void)hipStreamSynchronize(sp->diffuse_ws->stream);
    return s;
}

}  // namespace as
