// Connected components of the item graph (section 5.25): the classes of the transitive closure of the
// stored CSR's kept entries -- every entry, or with a threshold t the entries with dist <= t (a NaN dist is never kept under a
// threshold) -- each item labelled with the smallest item id of its class.
// State: one int32 parent[n], parent[i] = i at the start.  Two invariants hold at every moment, whatever the order in which the
// atomics land and however stale a read is: (I1) parent[x] <= x, and parent[x] only ever decreases; (I2) parent[x] lies in x's
// component.  A round is two launches on the work's stream:
//   hook      streams the CSR; for a kept entry (i, j) it reads a = parent[i], b = parent[j] and, if they differ, does
//             atomicMin(&parent[max(a, b)], min(a, b)).  Both values lie in the component of the entry (I2), the smaller is written
//             below the larger (I1).
//   compress  every item chases parent to a root (parent[r] == r) and stores it.  No launch of compress lowers a root, so after
//             it every parent IS a root.
// The hook raises the round's flag when it saw a != b at any kept entry: one atomic per block at most.  Every value in parent
// during a hook launch is a value it held at the launch's start (the hook writes only values it read), that is a root r with
// parent[r] = r; so the first lane to see a != b at max(a, b) = r does lower parent[r], and "an entry with unequal parents was
// seen" is the same event, for the launch as a whole, as "something was lowered".  The host reads the flag once per round (a
// pinned copy on the stream) and stops after the first round whose hook raised nothing.  Then nothing was written during that
// launch, so every read in it was of the launch's start: every kept entry has equal parents, every parent is a root r, r <= each
// member (I1), r is a member (I2) and members of one class share it: r is the class's smallest id.  Nothing rests on one lane
// seeing another's write inside a launch: a stale read costs a round at most; the kernel boundary and the host's read decide.
// The statistics (sizes by integer atomics at parent[i], then one reduction with integer sum, min and max) are order-free.
// Entry points: as_api.hip (as_graph_components, as_graph_components_sweep, as_components_counters).
#include <algorithm>
#include <cmath>
#include <vector>

#include "as_diffuse.hpp"

namespace as {

namespace {

constexpr int CC_STAT_WORDS = 6;   // CcStat as 64-bit words: what a stage's memset zeroes

// what a stage leaves on the device and the host reads: 48 bytes at the start of their allocation
struct CcStat {
    unsigned long long flag;      // the number of the last round whose hook saw unequal parents (rounds count from 1)
    unsigned long long kept;      // kept entries, counted by the stage's first hook
    unsigned long long count;     // components
    unsigned long long isolated;  // components of one item
    unsigned long long key;       // max over the labels of (size << 32 | ~label): the largest size, the smallest label that has it
    unsigned long long pad;
};
static_assert(sizeof(CcStat) == 8 * CC_STAT_WORDS, "CcStat is six 64-bit words");

struct CcHookArgs {
    const int64_t* indptr;    // [n + 1]
    const int32_t* indices;   // [nnz]
    const double* dist;       // [nnz]; not read without a threshold
    int32_t* parent;          // [n]
    CcStat* stat;
    int64_t n;
    double t;
    unsigned long long round;
    int count;                // the stage's first round: add the kept entries to stat->kept
};

__global__ __launch_bounds__(DIF_THREADS) void cc_init_kernel(int32_t* parent, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DIF_THREADS) parent[i] = (int32_t)i;
}

// A block owns groups of DIF_THREADS consecutive rows (grid-stride over the groups), as the C = 1 step of the diffusion does: the
// entries of a group are one contiguous run of the CSR, read coalesced a lane per entry, so a hub row of thousands of entries is
// spread over the block like any other run.  The group's row starts sit in LDS; an entry finds its row by bisection there.
template <bool FILTER>
__global__ __launch_bounds__(DIF_THREADS) void cc_hook_kernel(CcHookArgs a) {
    __shared__ int64_t s_ptr[DIF_THREADS + 1];
    __shared__ unsigned long long s_kept;
    __shared__ int s_seen;
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_kept = 0;
        s_seen = 0;
    }
    unsigned long long kept = 0;
    bool seen = false;
    const int64_t groups = (a.n + DIF_THREADS - 1) / DIF_THREADS;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t first = g * DIF_THREADS;
        const int nr = (int)(first + DIF_THREADS < a.n ? DIF_THREADS : a.n - first);
        __syncthreads();   // the last group's row starts are read before these are written
        for (int r = tid; r <= nr; r += DIF_THREADS) s_ptr[r] = a.indptr[first + r];
        __syncthreads();
        const int64_t e0 = s_ptr[0], e1 = s_ptr[nr];
        for (int64_t e = e0 + tid; e < e1; e += DIF_THREADS) {
            if (FILTER && !(a.dist[e] <= a.t)) continue;   // (a NaN fails the comparison)
            ++kept;
            int lo = 0, hi = nr;   // s_ptr[lo] <= e < s_ptr[hi]: the row is the last one that starts at or before e
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_ptr[mid] <= e) lo = mid;
                else hi = mid;
            }
            const int32_t pa = a.parent[first + lo], pb = a.parent[a.indices[e]];
            if (pa != pb) {
                atomicMin(&a.parent[pa > pb ? pa : pb], pa > pb ? pb : pa);
                seen = true;
            }
        }
    }
    if (seen) s_seen = 1;   // (every writer stores the same value)
    if (a.count) {
        for (int o = 32; o > 0; o >>= 1) kept += __shfl_down(kept, o);
        if ((tid & 63) == 0 && kept) atomicAdd(&s_kept, kept);
    }
    __syncthreads();
    if (tid == 0) {
        if (s_seen) atomicMax(&a.stat->flag, a.round);
        if (a.count && s_kept) atomicAdd(&a.stat->kept, s_kept);
    }
}

// parent[x] <- the root of x.  The chase reads and the store are relaxed agent-scope atomics: a root another lane has just stored
// is met in the second-level cache instead of a stale line of this CU's, which shortens long chains (ids that follow a path);
// the result does not need it -- a stale value is an ancestor too (I1, I2), and the chase ends at a root either way.
__global__ __launch_bounds__(DIF_THREADS) void cc_compress_kernel(int32_t* parent, int64_t n) {
    for (int64_t x = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; x < n; x += (int64_t)gridDim.x * DIF_THREADS) {
        int32_t r = parent[x];
        if (r == (int32_t)x) continue;
        for (;;) {
            const int32_t p = __hip_atomic_load(&parent[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (p == r) break;
            r = p;
        }
        __hip_atomic_store(&parent[x], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// size[parent[i]] += 1, one int32 atomic per item.  (One atomic per run of equal neighbouring labels of a wave, the shape of grouped
// search's pick kernels, was measured at 1M items and was not faster -- section 5.25 -- so it is not built.)
__global__ __launch_bounds__(DIF_THREADS) void cc_sizes_kernel(const int32_t* __restrict__ parent, int64_t n, int32_t* size) {
    for (int64_t i = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DIF_THREADS) atomicAdd(&size[parent[i]], 1);
}

// count, isolated and key of CcStat from the sizes: per lane, per wave, per block, then one atomic each per block
__global__ __launch_bounds__(DIF_THREADS) void cc_reduce_kernel(const int32_t* __restrict__ size, int64_t n, CcStat* stat) {
    __shared__ unsigned long long s_count, s_iso, s_key;
    if (threadIdx.x == 0) s_count = s_iso = s_key = 0;
    __syncthreads();
    unsigned long long count = 0, iso = 0, key = 0;
    for (int64_t i = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DIF_THREADS) {
        const int32_t s = size[i];
        if (s <= 0) continue;
        ++count;
        iso += s == 1;
        const unsigned long long k = ((unsigned long long)(uint32_t)s << 32) | (0xffffffffu - (uint32_t)i);
        key = k > key ? k : key;
    }
    for (int o = 32; o > 0; o >>= 1) {
        count += __shfl_down(count, o);
        iso += __shfl_down(iso, o);
        const unsigned long long k = __shfl_down(key, o);
        key = k > key ? k : key;
    }
    if ((threadIdx.x & 63) == 0 && count) {
        atomicAdd(&s_count, count);
        atomicAdd(&s_iso, iso);
        atomicMax(&s_key, key);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_count) {
        atomicAdd(&stat->count, s_count);
        if (s_iso) atomicAdd(&stat->isolated, s_iso);
        atomicMax(&stat->key, s_key);
    }
}

unsigned cc_grid(const DiffuseWork* w, int64_t blocks) { return diffuse_grid(std::min<int64_t>(blocks, (int64_t)w->cus * DIF_BLOCKS_PER_CU)); }

// the device time between two recorded events, added to *us
as_status add_elapsed(hipEvent_t e0, hipEvent_t e1, double* us) {
    float ms = 0.0f;
    AS_HIP(hipEventElapsedTime(&ms, e0, e1));
    *us += (double)ms * 1e3;
    return AS_OK;
}

// One threshold on the state `parent` holds (a cold start, or the fixed point of a smaller threshold: the kept sets are nested, so
// that state satisfies both invariants for this one, and the fixed point is unique): the rounds, then the statistics -> *info.
// labels_host: the 4 n bytes of labels cross too.
as_status cc_stage(DiffuseWork* w, const as_graph* gr, const double* t, int32_t* labels_host, as_components_info* info, bool timing,
                   int64_t* counts) {
    const int64_t n = gr->n;
    int32_t* parent = w->cc_parent;
    CcStat* stat = (CcStat*)(unsigned long long*)w->cc_stat_d;
    CcStat* host = (CcStat*)(unsigned long long*)w->cc_stat_h;
    const unsigned rgrid = cc_grid(w, (n + DIF_THREADS - 1) / DIF_THREADS);
    AS_HIP(hipMemsetAsync(stat, 0, sizeof(CcStat), w->stream));
    AS_HIP(hipMemsetAsync((int32_t*)w->cc_size, 0, sizeof(int32_t) * (size_t)n, w->stream));
    CcHookArgs a;
    a.indptr = gr->indptr; a.indices = gr->indices; a.dist = gr->dist; a.parent = parent; a.stat = stat; a.n = n; a.t = t ? *t : 0.0;
    int64_t rounds = 0;
    for (;;) {
        a.round = (unsigned long long)++rounds;
        a.count = rounds == 1;
        if (timing) AS_HIP(hipEventRecord(w->cc_ev.e[0], w->stream));
        if (t) hipLaunchKernelGGL(cc_hook_kernel<true>, dim3(rgrid), dim3(DIF_THREADS), 0, w->stream, a);
        else hipLaunchKernelGGL(cc_hook_kernel<false>, dim3(rgrid), dim3(DIF_THREADS), 0, w->stream, a);
        if (timing) AS_HIP(hipEventRecord(w->cc_ev.e[1], w->stream));
        hipLaunchKernelGGL(cc_compress_kernel, dim3(rgrid), dim3(DIF_THREADS), 0, w->stream, parent, n);
        if (timing) AS_HIP(hipEventRecord(w->cc_ev.e[2], w->stream));
        AS_HIP(hipGetLastError());
        AS_HIP(hipMemcpyAsync(&host->flag, &stat->flag, sizeof(unsigned long long), hipMemcpyDeviceToHost, w->stream));
        AS_HIP(hipStreamSynchronize(w->stream));
        counts[0] += 1;   // hook launches
        counts[1] += 1;   // compress launches
        counts[2] += 1;   // host waits
        if (timing) {
            AS_TRY(add_elapsed(w->cc_ev.e[0], w->cc_ev.e[1], &w->cc_us[0]));
            AS_TRY(add_elapsed(w->cc_ev.e[1], w->cc_ev.e[2], &w->cc_us[1]));
        }
        if (host->flag != (unsigned long long)rounds) break;   // this round's hook saw no entry with unequal parents
    }
    if (timing) AS_HIP(hipEventRecord(w->cc_ev.e[0], w->stream));
    hipLaunchKernelGGL(cc_sizes_kernel, dim3(rgrid), dim3(DIF_THREADS), 0, w->stream, (const int32_t*)parent, n, (int32_t*)w->cc_size);
    hipLaunchKernelGGL(cc_reduce_kernel, dim3(rgrid), dim3(DIF_THREADS), 0, w->stream, (const int32_t*)w->cc_size, n, stat);
    if (timing) AS_HIP(hipEventRecord(w->cc_ev.e[1], w->stream));
    AS_HIP(hipGetLastError());
    AS_HIP(hipMemcpyAsync(host, stat, sizeof(CcStat), hipMemcpyDeviceToHost, w->stream));
    if (labels_host) AS_HIP(hipMemcpyAsync(labels_host, parent, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, w->stream));
    AS_HIP(hipStreamSynchronize(w->stream));
    counts[2] += 1;
    if (timing) AS_TRY(add_elapsed(w->cc_ev.e[0], w->cc_ev.e[1], &w->cc_us[2]));
    w->cc_us[3] += (double)rounds;
    if (info) {
        info->count = (int64_t)host->count;
        info->largest = (int64_t)(host->key >> 32);
        info->largest_label = (int64_t)(0xffffffffu - (uint32_t)(host->key & 0xffffffffu));
        info->isolated = (int64_t)host->isolated;
        info->edges_kept = (int64_t)host->kept;
        info->rounds = rounds;
    }
    return AS_OK;
}

as_status cc_run(const as_space* sp, const as_graph* gr, const double* ts, int32_t nt, int32_t* labels_host, as_components_info* info,
                 int64_t* counts) {
    const int64_t n = gr->n;
    DiffuseWork* w = nullptr;
    AS_TRY(diffuse_work_get(sp, &w));
    const bool timing = diffuse_timing();
    for (int i = 0; i < 4; ++i) w->cc_us[i] = 0.0;
    AS_TRY(reserve_or_err(w->cc_parent, n, "components parents"));
    AS_TRY(reserve_or_err(w->cc_size, n, "components sizes"));
    AS_TRY(reserve_or_err(w->cc_stat_d, CC_STAT_WORDS, "components statistics"));
    AS_TRY(reserve_or_err(w->cc_stat_h, CC_STAT_WORDS, "components pinned statistics"));
    if (timing && !w->cc_ev.e[0]) AS_HIP(w->cc_ev.create());
    hipLaunchKernelGGL(cc_init_kernel, dim3(cc_grid(w, (n + DIF_THREADS - 1) / DIF_THREADS)), dim3(DIF_THREADS), 0, w->stream, (int32_t*)w->cc_parent, n);
    if (!ts) return cc_stage(w, gr, nullptr, labels_host, info, timing, counts);
    // the distinct thresholds ascending, each from the last one's fixed point; duplicates and the caller's order on the host
    std::vector<int> order((size_t)nt);
    for (int i = 0; i < nt; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return ts[x] < ts[y]; });
    for (int i = 0; i < nt; ++i) {
        const int at = order[(size_t)i];
        if (i > 0 && ts[at] == ts[order[(size_t)i - 1]]) {
            if (info) info[at] = info[order[(size_t)i - 1]];
            continue;
        }
        AS_TRY(cc_stage(w, gr, &ts[at], labels_host, info ? info + at : nullptr, timing, counts));
    }
    return AS_OK;
}

}  // namespace

double components_kernel_us(const DiffuseWork* w, int part) { return w && part >= 0 && part < 4 ? w->cc_us[part] : 0.0; }

// (a failed run leaves nothing on the stream when the caller releases the lock)
as_status components_run(const as_space* sp, const as_graph* gr, const double* ts, int32_t nt, int32_t* labels_host, as_components_info* info,
                         int64_t* counts) {
    if (gr->n <= 0) {
        for (int i = 0; info && i < (ts ? nt : 1); ++i) info[i] = as_components_info{0, 0, 0, 0, 0, 0};
        return AS_OK;
    }
    as_status s;
    try {
        s = cc_run(sp, gr, ts, nt, labels_host, info, counts);
    } catch (const std::bad_alloc&) {
        set_err("components: out of host memory");
        s = AS_ENOMEM;
    }
    if (s != AS_OK && sp->diffuse_ws) (void)hipStreamSynchronize(sp->diffuse_ws->stream);
    return s;
}

}  // namespace as
