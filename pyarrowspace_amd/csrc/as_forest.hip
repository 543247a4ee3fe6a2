// Minimum spanning forest of the item graph (section 5.26): over the distinct undirected edges {u < v} of
// the stored CSR, each weighted with the smaller of its two stored dists (a NaN ignored; NaN if both are), under the total order
// (w ascending with NaN after +inf, then u, then v), the unique minimum spanning forest -- by Boruvka rounds on the device.
// State: parent[n] (every entry a root between rounds: parent[parent[x]] == parent[x]), hook[n] (hook[r] == r for a root), per
// row a candidate (rkey, rj), per root the minimum of its rows' candidates (rootkey, rootuv), per item an output slot.
// A call writes wkey[e], the order-preserving 64-bit image of entry e's undirected weight, once; then a round is four launches:
//   (a) rowmin    a sub-wave of W lanes per row: the smallest (wkey, j) over the entries with parent[j] != parent[i]; the row's
//                 candidate is stored and its wkey goes to the root with one 64-bit atomicMin.  A row without such an entry is
//                 marked dead: classes only grow, so it never has one again, and no later round reads its entries.
//   (b) pick      a lane per row: a row whose candidate's wkey IS its root's minimum does atomicMin of (u << 32 | v) there.  For a
//                 fixed row ascending j is ascending (u, v), so after (a) and (b) a root holds the minimum outgoing edge of its
//                 class in the total order -- a minimum of integers, whatever order the atomics land in.
//   (c) link      a lane per root r with a candidate: s is the root across the edge.  If s holds the same edge and r < s, r stays
//                 a root; else r writes the edge into slot r and hook[r] = s.  The minimum outgoing edge of a class belongs to the
//                 forest (the cut property under a total order), the picks of a round can only close the two-cycles broken here
//                 (along a cycle of picks the edges would strictly decrease), and a root that emits stops being one: slot r is
//                 written at most once per call.  (c) reads parent and the roots' words and writes hook and slots only.
//   (d) compress  a lane per item chases hook from parent[x] to a root, stores it in parent[x], and clears the item's root words.
// (c) raises the round's number in a flag, one atomic per block at most, when a root had a candidate; the host reads the flag
// once per round through pinned memory and stops after the first round without one.  Every round at least halves the classes
// of a component that still has two: rounds <= ceil(log2(largest component)) + 1.
// Emit: the used slots are compacted in slot order by ballot ranks under a prefix over the counts of 256-slot chunks (no atomics),
// the wkey decoded to fp64 bits; 16 bytes per edge cross.  The sort by the total order, when asked, is the host's.
// Nothing here depends on the grid, on W or on the order of the atomics: every value a round leaves is a minimum over a set the
// graph and the state at the round's start define.
// Entry points: as_api.hip (as_graph_forest, as_forest_counters, as_forest_kernel_us).
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstring>
#include <vector>

#include "as_diffuse.hpp"

namespace as {

namespace {

constexpr unsigned long long FR_EMPTY = ~0ull;                  // no candidate, an unused slot: above every image
constexpr int32_t FR_DEAD = -2;    // rj of a row that has no entry into another class
constexpr int FR_CHUNK = DIF_THREADS;   // slots of an emit chunk

struct FrStat {
    unsigned long long flag;    // the number of the last round in which a root had a candidate (rounds count from 1)
    unsigned long long edges;   // used slots, written by the scan
};

struct FrArgs {
    const int64_t* indptr;    // [n + 1]
    const int32_t* indices;   // [nnz]
    const unsigned long long* wkey;   // [nnz]
    int32_t* parent;          // [n]
    int32_t* hook;            // [n]
    int32_t* rj;              // [n] the row's candidate column, FR_DEAD
    unsigned long long* rkey;      // [n] ... and its wkey
    unsigned long long* rootkey;   // [n] at a root: the smallest wkey of its rows' candidates, FR_EMPTY
    unsigned long long* rootuv;    // [n] at a root: the smallest (u << 32 | v) among the candidates of that wkey, FR_EMPTY
    unsigned long long* slotuv;    // [n] the edge root r emitted, FR_EMPTY
    unsigned long long* slotkey;   // [n] ... and its wkey
    FrStat* stat;
    int64_t n;
    unsigned long long round;
};

__global__ __launch_bounds__(DIF_THREADS) void fr_init_kernel(FrArgs a) {
    for (int64_t x = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; x < a.n; x += (int64_t)gridDim.x * DIF_THREADS) {
        a.parent[x] = (int32_t)x;
        a.hook[x] = (int32_t)x;
        a.rj[x] = -1;
        a.rootkey[x] = FR_EMPTY;
        a.rootuv[x] = FR_EMPTY;
        a.slotuv[x] = FR_EMPTY;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.stat->flag = 0;
        a.stat->edges = 0;
    }
}

}  // namespace

// (declared in as_diffuse.hpp: the shortest paths of as_geodesic.hip launch it too)
// wkey[e] = min(image of dist[e], image of the reverse entry's dist): FR_NAN lies above every number, so a NaN loses to one and
// two NaNs stay FR_NAN.  The rows of a group and the lane-per-entry layout are the components hook's; the reverse entry (j, i) is
// found by bisection in row j's ascending columns (S4 stores it; were it missing the entry's own dist would stand).
__global__ __launch_bounds__(DIF_THREADS) void fr_weights_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                                  const double* __restrict__ dist, unsigned long long* __restrict__ wkey,
                                                                  int64_t n) {
    __shared__ int64_t s_ptr[DIF_THREADS + 1];
    const int tid = threadIdx.x;
    const int64_t groups = (n + DIF_THREADS - 1) / DIF_THREADS;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t first = g * DIF_THREADS;
        const int nr = (int)(first + DIF_THREADS < n ? DIF_THREADS : n - first);
        __syncthreads();   // the last group's row starts are read before these are written
        for (int r = tid; r <= nr; r += DIF_THREADS) s_ptr[r] = indptr[first + r];
        __syncthreads();
        const int64_t e0 = s_ptr[0], e1 = s_ptr[nr];
        for (int64_t e = e0 + tid; e < e1; e += DIF_THREADS) {
            int lo = 0, hi = nr;   // s_ptr[lo] <= e < s_ptr[hi]: the row is the last one that starts at or before e
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_ptr[mid] <= e) lo = mid;
                else hi = mid;
            }
            const int32_t i = (int32_t)(first + lo), j = indices[e];
            unsigned long long key = forest_key(dist[e]);
            if (j >= 0 && (int64_t)j < n) {
                const int64_t r1 = indptr[(int64_t)j + 1];
                int64_t a = indptr[j], b = r1;   // the first entry of row j with a column >= i
                while (a < b) {
                    const int64_t mid = (a + b) >> 1;
                    if (indices[mid] < i) a = mid + 1;
                    else b = mid;
                }
                if (a < r1 && indices[a] == i) {
                    const unsigned long long other = forest_key(dist[a]);
                    key = other < key ? other : key;
                }
            }
            wkey[e] = key;
        }
    }
}

namespace {

// (a): W lanes per row, DIF_THREADS / W rows per block and trip.  The lanes of a sub-wave share the row, so every branch below
// is uniform over the lanes the cross-lane moves read.
template <int W>
__global__ __launch_bounds__(DIF_THREADS) void fr_rowmin_kernel(FrArgs a) {
    constexpr int ROWS = DIF_THREADS / W;
    const int sub = threadIdx.x / W, lane = threadIdx.x % W;
    const int64_t trips = (a.n + ROWS - 1) / ROWS;
    for (int64_t g = blockIdx.x; g < trips; g += gridDim.x) {
        const int64_t i = g * ROWS + sub;
        if (i >= a.n || a.rj[i] == FR_DEAD) continue;
        const int32_t pi = a.parent[i];
        unsigned long long best = FR_EMPTY;
        int32_t bj = INT_MAX;
        const int64_t e1 = a.indptr[i + 1];
        for (int64_t e = a.indptr[i] + lane; e < e1; e += W) {   // a lane meets its columns ascending: `<` keeps the smallest j
            const int32_t j = a.indices[e];
            const unsigned long long k = a.wkey[e];
            if (k < best && a.parent[j] != pi) {
                best = k;
                bj = j;
            }
        }
        for (int o = W / 2; o > 0; o >>= 1) {
            const unsigned long long ok = __shfl_xor(best, o, W);
            const int32_t oj = __shfl_xor(bj, o, W);
            if (ok < best || (ok == best && oj < bj)) {
                best = ok;
                bj = oj;
            }
        }
        if (lane == 0) {
            if (best == FR_EMPTY) {
                a.rj[i] = FR_DEAD;
            } else {
                a.rkey[i] = best;
                a.rj[i] = bj;
                atomicMin(&a.rootkey[pi], best);
            }
        }
    }
}

// (b)
__global__ __launch_bounds__(DIF_THREADS) void fr_pick_kernel(FrArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * DIF_THREADS) {
        const int32_t j = a.rj[i];
        if (j < 0) continue;
        const int32_t pi = a.parent[i];
        if (a.rkey[i] != a.rootkey[pi]) continue;
        const uint32_t u = (uint32_t)((int32_t)i < j ? (int32_t)i : j), v = (uint32_t)((int32_t)i < j ? j : (int32_t)i);
        atomicMin(&a.rootuv[pi], ((unsigned long long)u << 32) | v);
    }
}

// (c)
__global__ __launch_bounds__(DIF_THREADS) void fr_link_kernel(FrArgs a) {
    __shared__ int s_seen;
    if (threadIdx.x == 0) s_seen = 0;
    __syncthreads();
    bool seen = false;
    for (int64_t x = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; x < a.n; x += (int64_t)gridDim.x * DIF_THREADS) {
        const int32_t r = (int32_t)x;
        const unsigned long long uv = a.rootuv[x];
        if (uv == FR_EMPTY || a.parent[x] != r) continue;   // (only a root's words are ever lowered)
        seen = true;
        const int32_t pu = a.parent[(int64_t)(uv >> 32)], pv = a.parent[(int64_t)(uv & 0xffffffffull)];
        const int32_t s = pu == r ? pv : pu;
        if (a.rootuv[s] == uv && r < s) continue;   // the two-cycle: the smaller root stays one
        a.slotuv[x] = uv;
        a.slotkey[x] = a.rootkey[x];
        a.hook[x] = s;
    }
    if (seen) s_seen = 1;   // (every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0 && s_seen) atomicMax(&a.stat->flag, a.round);
}

// (d): parent[x] <- the root hook leads to from parent[x].  The chase reads and the stores are relaxed agent-scope atomics, as in
// the components' compress: a root that another lane has just written into hook[y] shortens the chain for everyone behind y (the
// first round of a path in id order hangs every item on one chain).  Whatever a chase reads in hook[y] is an ancestor of y, and
// the hooks hold no cycle, so it ends at the root either way.
__global__ __launch_bounds__(DIF_THREADS) void fr_compress_kernel(FrArgs a) {
    for (int64_t x = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; x < a.n; x += (int64_t)gridDim.x * DIF_THREADS) {
        if (a.rootuv[x] != FR_EMPTY) {   // the words of this round's roots, for the next round
            a.rootuv[x] = FR_EMPTY;
            a.rootkey[x] = FR_EMPTY;
        }
        int32_t r = a.parent[x];
        for (;;) {
            const int32_t p = __hip_atomic_load(&a.hook[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (p == r) break;
            r = p;
        }
        if (a.parent[x] == r) continue;
        a.parent[x] = r;
        if (a.hook[x] != (int32_t)x) __hip_atomic_store(&a.hook[x], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// emit, first pass: the used slots of every chunk of FR_CHUNK slots
__global__ __launch_bounds__(DIF_THREADS) void fr_count_kernel(const unsigned long long* __restrict__ slotuv, int64_t n, int64_t* chunk) {
    __shared__ int s_wave[DIF_THREADS / 64];
    const int64_t chunks = (n + FR_CHUNK - 1) / FR_CHUNK;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t x = c * FR_CHUNK + threadIdx.x;
        const unsigned long long used = __ballot(x < n && slotuv[x] != FR_EMPTY);
        __syncthreads();   // the last chunk's counts are read before these are written
        if (lane_id() == 0) s_wave[threadIdx.x >> 6] = __popcll(used);
        __syncthreads();
        if (threadIdx.x == 0) {
            int sum = 0;
            for (int w = 0; w < DIF_THREADS / 64; ++w) sum += s_wave[w];
            chunk[c] = sum;
        }
    }
}

// ... the exclusive prefix of the chunk counts in place, by one block: a thread sums a run of chunks, thread 0 the 256 sums
__global__ __launch_bounds__(DIF_THREADS) void fr_scan_kernel(int64_t* chunk, int64_t chunks, FrStat* stat) {
    __shared__ int64_t s_sum[DIF_THREADS];
    const int64_t per = (chunks + DIF_THREADS - 1) / DIF_THREADS;
    const int64_t c0 = per * threadIdx.x < chunks ? per * threadIdx.x : chunks, c1 = c0 + per < chunks ? c0 + per : chunks;
    int64_t sum = 0;
    for (int64_t c = c0; c < c1; ++c) sum += chunk[c];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t at = 0;
        for (int t = 0; t < DIF_THREADS; ++t) {
            const int64_t v = s_sum[t];
            s_sum[t] = at;
            at += v;
        }
        stat->edges = (unsigned long long)at;
    }
    __syncthreads();
    int64_t at = s_sum[threadIdx.x];
    for (int64_t c = c0; c < c1; ++c) {
        const int64_t v = chunk[c];
        chunk[c] = at;
        at += v;
    }
}

// ... second pass: a used slot's place is its chunk's base, the used slots of the waves before it and its rank in its wave's ballot
__global__ __launch_bounds__(DIF_THREADS) void fr_write_kernel(const unsigned long long* __restrict__ slotuv,
                                                                const unsigned long long* __restrict__ slotkey, int64_t n,
                                                                const int64_t* __restrict__ chunk, int32_t* __restrict__ out_u,
                                                                int32_t* __restrict__ out_v, unsigned long long* __restrict__ out_w) {
    __shared__ int s_wave[DIF_THREADS / 64];
    const int64_t chunks = (n + FR_CHUNK - 1) / FR_CHUNK;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t x = c * FR_CHUNK + threadIdx.x;
        const unsigned long long uv = x < n ? slotuv[x] : FR_EMPTY;
        const unsigned long long used = __ballot(uv != FR_EMPTY);
        __syncthreads();
        if (lane_id() == 0) s_wave[threadIdx.x >> 6] = __popcll(used);
        __syncthreads();
        if (uv != FR_EMPTY) {   // (no `continue`: every lane of the block reaches the next trip's ballot and barriers together)
            int64_t at = chunk[c] + __popcll(used & ((1ull << lane_id()) - 1));
            for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) at += s_wave[w];
            out_u[at] = (int32_t)(uv >> 32);
            out_v[at] = (int32_t)(uv & 0xffffffffull);
            out_w[at] = forest_bits(slotkey[x]);
        }
    }
}

std::atomic<int> g_forest_row_lanes{16};

unsigned fr_grid(const DiffuseWork* w, int64_t blocks) { return diffuse_grid(std::min<int64_t>(blocks, (int64_t)w->cus * DIF_BLOCKS_PER_CU)); }

void fr_rowmin_launch(const DiffuseWork* w, const FrArgs& a, int lanes) {
    const int64_t trips = (a.n + DIF_THREADS / lanes - 1) / (DIF_THREADS / lanes);
    const unsigned grid = fr_grid(w, trips);
    if (lanes == 8) hipLaunchKernelGGL(fr_rowmin_kernel<8>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
    else if (lanes == 32) hipLaunchKernelGGL(fr_rowmin_kernel<32>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
    else hipLaunchKernelGGL(fr_rowmin_kernel<16>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
}

as_status fr_elapsed(hipEvent_t e0, hipEvent_t e1, double* us) {
    float ms = 0.0f;
    AS_HIP(hipEventElapsedTime(&ms, e0, e1));
    *us = (double)ms * 1e3;
    return AS_OK;
}

struct FrEdge {
    unsigned long long key;
    int32_t u, v;
};

as_status fr_run(const as_space* sp, const as_graph* gr, int sort, int32_t* u_host, int32_t* v_host, double* dist_host, as_forest_info* info,
                 int64_t* counts) {
    const int64_t n = gr->n, nnz = gr->nnz;
    const int64_t chunks = (n + FR_CHUNK - 1) / FR_CHUNK;
    DiffuseWork* w = nullptr;
    AS_TRY(diffuse_work_get(sp, &w));
    const bool timing = diffuse_timing();
    for (double& v : w->fr_us) v = 0.0;
    w->fr_wkey_serial = 0;
    AS_TRY(reserve_or_err(w->fr_wkey, nnz, "forest weights"));
    AS_TRY(reserve_or_err(w->fr_words, 6 * n + chunks, "forest words"));
    AS_TRY(reserve_or_err(w->fr_ints, 5 * n, "forest ids"));
    AS_TRY(reserve_or_err(w->fr_stat_d, 2, "forest flag"));
    AS_TRY(reserve_or_err(w->fr_stat_h, 2, "forest pinned flag"));
    if (timing && !w->fr_ev.e[0]) AS_HIP(w->fr_ev.create());
    unsigned long long* words = w->fr_words;
    int32_t* ints = w->fr_ints;
    FrStat* stat = (FrStat*)(unsigned long long*)w->fr_stat_d;
    FrStat* host = (FrStat*)(unsigned long long*)w->fr_stat_h;
    FrArgs a;
    a.indptr = gr->indptr; a.indices = gr->indices; a.wkey = w->fr_wkey; a.stat = stat; a.n = n; a.round = 0;
    a.rkey = words; a.rootkey = words + n; a.rootuv = words + 2 * n; a.slotuv = words + 3 * n; a.slotkey = words + 4 * n;
    unsigned long long* out_w = words + 5 * n;
    int64_t* chunk = (int64_t*)(words + 6 * n);
    a.parent = ints; a.hook = ints + n; a.rj = ints + 2 * n;
    int32_t* out_u = ints + 3 * n;
    int32_t* out_v = ints + 4 * n;
    const unsigned igrid = fr_grid(w, (n + DIF_THREADS - 1) / DIF_THREADS);
    const int lanes = g_forest_row_lanes.load(std::memory_order_relaxed);
    hipEvent_t* ev = w->fr_ev.e;

    if (timing) AS_HIP(hipEventRecord(ev[0], w->stream));
    hipLaunchKernelGGL(fr_init_kernel, dim3(igrid), dim3(DIF_THREADS), 0, w->stream, a);
    if (nnz > 0) hipLaunchKernelGGL(fr_weights_kernel, dim3(igrid), dim3(DIF_THREADS), 0, w->stream, (const int64_t*)gr->indptr,
                                    (const int32_t*)gr->indices, (const double*)gr->dist, (unsigned long long*)w->fr_wkey, n);
    if (timing) AS_HIP(hipEventRecord(ev[1], w->stream));
    AS_HIP(hipGetLastError());
    w->fr_wkey_serial = gr->serial;   // the images are this graph's: the shortest paths read them without a launch of their own
    counts[1] += nnz > 0 ? 2 : 1;
    if (timing) {
        AS_HIP(hipStreamSynchronize(w->stream));
        AS_TRY(fr_elapsed(ev[0], ev[1], &w->fr_us[4]));
    }
    int64_t rounds = 0;
    for (;;) {
        a.round = (unsigned long long)++rounds;
        if (timing) AS_HIP(hipEventRecord(ev[0], w->stream));
        fr_rowmin_launch(w, a, lanes);
        if (timing) AS_HIP(hipEventRecord(ev[1], w->stream));
        hipLaunchKernelGGL(fr_pick_kernel, dim3(igrid), dim3(DIF_THREADS), 0, w->stream, a);
        if (timing) AS_HIP(hipEventRecord(ev[2], w->stream));
        hipLaunchKernelGGL(fr_link_kernel, dim3(igrid), dim3(DIF_THREADS), 0, w->stream, a);
        if (timing) AS_HIP(hipEventRecord(ev[3], w->stream));
        hipLaunchKernelGGL(fr_compress_kernel, dim3(igrid), dim3(DIF_THREADS), 0, w->stream, a);
        if (timing) AS_HIP(hipEventRecord(ev[4], w->stream));
        AS_HIP(hipGetLastError());
        AS_HIP(hipMemcpyAsync(&host->flag, &stat->flag, sizeof(unsigned long long), hipMemcpyDeviceToHost, w->stream));
        AS_HIP(hipStreamSynchronize(w->stream));
        counts[0] += 1;
        counts[1] += 4;
        counts[2] += 1;
        if (timing)
            for (int k = 0; k < 4; ++k) {
                double us = 0.0;
                AS_TRY(fr_elapsed(ev[k], ev[k + 1], &us));
                w->fr_us[k] += us;
                if (rounds <= FR_TIMED_ROUNDS) w->fr_us[8 + 4 * (rounds - 1) + k] = us;
            }
        if (host->flag != (unsigned long long)rounds) break;   // no root had a candidate in this round
    }
    if (timing) AS_HIP(hipEventRecord(ev[0], w->stream));
    const unsigned cgrid = fr_grid(w, chunks);
    hipLaunchKernelGGL(fr_count_kernel, dim3(cgrid), dim3(DIF_THREADS), 0, w->stream, (const unsigned long long*)a.slotuv, n, chunk);
    hipLaunchKernelGGL(fr_scan_kernel, dim3(1), dim3(DIF_THREADS), 0, w->stream, chunk, chunks, stat);
    hipLaunchKernelGGL(fr_write_kernel, dim3(cgrid), dim3(DIF_THREADS), 0, w->stream, (const unsigned long long*)a.slotuv,
                       (const unsigned long long*)a.slotkey, n, (const int64_t*)chunk, out_u, out_v, out_w);
    if (timing) AS_HIP(hipEventRecord(ev[1], w->stream));
    AS_HIP(hipGetLastError());
    AS_HIP(hipMemcpyAsync(&host->edges, &stat->edges, sizeof(unsigned long long), hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[1] += 3;
    counts[2] += 1;
    if (timing) AS_TRY(fr_elapsed(ev[0], ev[1], &w->fr_us[5]));
    const int64_t m = (int64_t)host->edges;
    if (m < 0 || m >= n) {
        set_err("forest: the device reported %lld edges for %lld items", (long long)m, (long long)n);
        return AS_EHIP;
    }
    if (m > 0) {
        AS_HIP(hipMemcpyAsync(u_host, out_u, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, w->stream));
        AS_HIP(hipMemcpyAsync(v_host, out_v, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, w->stream));
        AS_HIP(hipMemcpyAsync(dist_host, out_w, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, w->stream));
        AS_HIP(hipStreamSynchronize(w->stream));
        counts[2] += 1;
    }
    if (sort && m > 1) {   // the total order on the host: (image of w, u, v)
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<FrEdge> edges((size_t)m);
        for (int64_t e = 0; e < m; ++e) edges[(size_t)e] = FrEdge{forest_key(dist_host[e]), u_host[e], v_host[e]};
        std::sort(edges.begin(), edges.end(), [](const FrEdge& x, const FrEdge& y) {
            return x.key != y.key ? x.key < y.key : (x.u != y.u ? x.u < y.u : x.v < y.v);
        });
        for (int64_t e = 0; e < m; ++e) {
            const unsigned long long bits = forest_bits(edges[(size_t)e].key);
            memcpy(&dist_host[e], &bits, sizeof(bits));
            u_host[e] = edges[(size_t)e].u;
            v_host[e] = edges[(size_t)e].v;
        }
        w->fr_us[6] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    w->fr_us[7] = (double)rounds;
    if (info) *info = as_forest_info{m, n - m, rounds};
    return AS_OK;
}

}  // namespace

void set_forest_row_lanes(int v) { g_forest_row_lanes.store(v == 8 || v == 32 ? v : 16, std::memory_order_relaxed); }

double forest_kernel_us(const DiffuseWork* w, int part) { return w && part >= 0 && part < 8 + 4 * FR_TIMED_ROUNDS ? w->fr_us[part] : 0.0; }

// (a failed run leaves nothing on the stream when the caller releases the lock)
as_status forest_run(const as_space* sp, const as_graph* gr, int sort, int32_t* u_host, int32_t* v_host, double* dist_host, as_forest_info* info,
                     int64_t* counts) {
    if (gr->n <= 0) {
        if (info) *info = as_forest_info{0, 0, 0};
        return AS_OK;
    }
    as_status s;
    try {
        s = fr_run(sp, gr, sort, u_host, v_host, dist_host, info, counts);
    } catch (const std::bad_alloc&) {
        set_err("forest: out of host memory");
        s = AS_ENOMEM;
    }
    if (s != AS_OK && sp->diffuse_ws) (void)hipStreamSynchronize(sp->diffuse_ws->stream);
    return s;
}

}  // namespace as
