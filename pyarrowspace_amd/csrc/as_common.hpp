// Shared host/device definitions for the gfx950 hot path (not part of the C ABI).
#pragma once
#include <memory>
#include <atomic>
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "arrowspace_hip.h"

namespace as {

constexpr int WAVE = 64;
constexpr int ROW_TILE = 256;   // rows of the item matrix are padded to a multiple of this
constexpr int COL_PAD = 32;     // feature dimension is padded to a multiple of this (floats)
constexpr double TAU_MIN = 1e-12;
constexpr int MAX_LIST = 64;    // widest wave-resident candidate list of one slot per lane (WaveList; WaveList2 holds two)
constexpr int MAX_KLIST = 128;  // widest k-NN candidate list (k + 8 <= 128)

// ---------------------------------------------------------------- errors
std::string& err_slot();
void set_err(const char* fmt, ...);
bool debug_enabled();
void dbg(const char* fmt, ...);

#define AS_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t _e = (call);                                                               \
        if (_e != hipSuccess) {                                                               \
            ::as::set_err("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
            return AS_EHIP;                                                                   \
        }                                                                                     \
    } while (0)

#define AS_TRY(call)                    \
    do {                                \
        as_status _s = (call);          \
        if (_s != AS_OK) return _s;     \
    } while (0)

}  // namespace as

namespace as { struct SubsetWork; struct ListsWork; struct RangeWork; struct DiverseWork; struct FusedWork; struct GroupedWork; struct MaxsimWork; struct MaxsimListsWork; struct DiffuseWork; }
struct as_subset;

// ---------------------------------------------------------------- handles
// HBM layout: x32 is the scan/MFMA operand, [np][dp] fp32,
// zero padded so that every tile load is a full 16-byte vector inside the allocation.
struct as_space {
    int device = 0;
    int64_t n = 0, d = 0, np = 0, dp = 0;
    float* x32 = nullptr;     // [np][dp]
    mutable float* xs = nullptr;  // [np][dp] bf16 head + tail image of x32 (as_k2bf.hip), made by the first k-NN pass; null until then
    // int8 two-digit image (as_k2bf.hip, quant_rows_i8): x ~ s_i (128 a1 + a2) / 16256, per row and 64-column slab 64 bytes of
    // a1 then 64 of a2 ([np + 256][dp8 * 2] bytes, dp8 = dp rounded up to 64); fa8[i] = s_i sqrt(128) / 16256; coef8 = the
    // error coefficient its products carry (from max_i s_i / |x_i| and max_i |x_i|_1 / |x_i|); k2_i8: the k-NN pass in
    // flight runs on it (set and cleared by knn_rows: err_coef follows it)
    mutable void* x8 = nullptr;
    mutable void* x8h = nullptr;   // the HIGH digits alone, planar ([np + 256][dp8] bytes): the single-query scan's coarse operand (space_i8h_image)
    mutable float* fa8 = nullptr;
    mutable double coef8 = 0.0;
    // ring build (one process per GPU): the ranks agreed to run the block passes on the int8 images (as_ring_i8_set); the
    // coefficient of a product of rows of two shards from the ring-wide maxima of U and V
    int ring_i8 = 0;
    double ring_u8 = 0.0, ring_v8 = 0.0, ring_coef8 = 0.0;
    mutable double uq_est = 0.0, vq_est = 0.0;   // batched int8 pass: 1.15 x the queries' measured residue norms of the previous passes (as_search.hip, host_batch_coef)
    mutable double u8max = 0.0, v8max = 0.0;   // max_i s_i |theta_i|_2 / (16256 |x_i|), max_i s_i |a2_i|_2 / (16256 |x_i|)
    mutable int x8_bad = 0;           // 1: non-finite items (the image exists but cannot be used), 2: no memory for the image (not retried)
    // image state for readers that do not take imu: 0 nothing decided, 1 x8 / fa8 / coef8 published (or x8_bad set): read-only from now on
    mutable std::atomic<int> x8_ready{0};
    mutable std::atomic<int> x8h_ready{0};   // ... the planar high digits: 1 x8h published, 2 not available (no memory)
    // NIBBLE tiles (as_build.hip, space_nib_image): the items quantised afresh to 4 bits, x ~ (lv + 1/2) t_i with lv in [-8, 7], one
    // KiB per 64 consecutive rows and 32-column chunk ([tile][chunk][64 rows][16 bytes], dp8 / 32 chunks; column 2 j in the low
    // nibble of byte j, column 2 j + 1 in the high one); fa4[i] = t_i; r4max = max_i |x_i - x~_i| / |x_i|, rounded up
    mutable void* x4 = nullptr;
    mutable float* fa4 = nullptr;
    mutable double r4max = 0.0;
    mutable std::atomic<int> x4_ready{0};    // 1 x4 / fa4 / r4max published, 2 not available (no memory, a failed build, a zero or non-finite row)
    // as_search_counters [6], [7]: single-query scans that read the nibble tiles, and those of them that were redone on the 8-bit tiles
    mutable std::atomic<int64_t> nib_count[2] = {};
    mutable std::mutex imu;           // makes the images (first use), per space
    mutable int k2_i8 = 0;
    mutable int k2_last_pipe = -1;   // matrix pipe of the last k-NN pass on this space: 0 fp32, 1 bf16 head + tail, 2 int8 two digits (as_space_knn_pipe)
    int64_t dp8 = 0;
    double* x64 = nullptr;    // [n][d] or null when the items are exactly fp32-representable
    double* n64 = nullptr;    // [n] squared norms (fp64, from the fp64 items)
    float* n32 = nullptr;     // [np] squared norms rounded to fp32 (0 on pad rows)
    float* inorm32 = nullptr; // [np] 1/|x| (0 for zero rows / pad rows)
    double* lam64 = nullptr;  // [n] lambdas (written by as_graph_from_knn)
    float* lam32 = nullptr;   // [np]
    int64_t row_offset = 0;   // global index of row 0 (a rank's shard of a row-sharded index); 0 for a whole index
    double nmax = 0.0;        // max squared norm
    int lossless = 0;         // items exactly representable in fp32
    as_opts opts{};
    hipStream_t stream = nullptr;
    // as_search is re-entrant across host threads: a pool of single-query workspaces (own stream, buffers, pinned results
    // each), lazily grown up to QPOOL; a call takes a free one under qmu and runs WITHOUT the lock, so one thread's scan
    // overlaps another's finish kernel and host turnaround.  qcache == qpool[0] (what a single thread ever uses).
    static constexpr int QPOOL = 4;
    mutable as_query* qpool[QPOOL] = {nullptr, nullptr, nullptr, nullptr};
    mutable bool qbusy[QPOOL] = {false, false, false, false};
    mutable std::condition_variable qcv;
    mutable std::mutex bmu;                   // the batched workspaces below (as_search_batch calls are serialised)
    mutable as_query* qcache = nullptr;       // lazily created by as_search
    mutable const as_graph* qcache_gr = nullptr;
    mutable as_query* qcache_b = nullptr;     // batched workspace (QUERY_BATCH slots), lazily created
    mutable as_query* qcache_b2 = nullptr;    // its twin: the two launch their passes as a PAIR that shares one scan (search_batch_launch_pair)
    mutable as_query* qcache_b3 = nullptr;    // a second pair (calls of more than 64 queries): one pair scans while the other's selection and
    mutable as_query* qcache_b4 = nullptr;    // finish kernels run and its results are read
    mutable std::atomic<long long> batch_dual_scans{0};   // scans that served two workspaces' passes (as_batch_counters)
    mutable const as_graph* qcache_b_gr = nullptr;
    mutable std::mutex qmu;
    // Gang scans (as_search.hip, gang_launch): single queries of host threads that arrive together share ONE pass over the tiles
    // of the coarse image.  active_callers: threads inside as_search on this space right now; gang_hint > 0: two or more were seen
    // within the last 64 searches (a lone thread never lingers); gang_width: the most seen at once lately; gang_open: the gang
    // that is gathering members (under gmu).
    mutable std::mutex gmu;
    mutable std::atomic<int> active_callers{0};
    mutable std::atomic<int> gang_hint{0};
    mutable std::atomic<int> gang_width{1};
    mutable std::atomic<unsigned> gang_tick{0};
    mutable std::shared_ptr<struct as_gang> gang_open;
    // one shared scan at a time, in the order the gangs were opened: the ticket of the next gang to open / to launch, and the event
    // behind the scan launched last (a workspace's gang_ev)
    mutable int64_t gang_seq_next = 0;                 // under gmu
    mutable std::atomic<int64_t> gang_seq_launched{0};
    mutable std::atomic<hipEvent_t> last_scan_ev{nullptr};
    mutable int64_t gang_scans[5] = {0, 0, 0, 0, 0};   // scans launched with 1 .. 4 members (index = members; under gmu)
    // host-prepared single-query scans that did NOT take the shared path, by first reason: [0] no concurrent callers lately, [1] the
    // search is not one for the fused tail (tau < 0.4, crowded candidates lately, ...), [2] not a coarse scan of the 8-bit tiles (the two-digit image, or a search prepared for the nibble tiles), [3] per-search
    // state still to be reset on the workspace's stream, [4] per-launch timing on, [5] a row range
    mutable std::atomic<int64_t> gang_skip[6] = {};
    // as_search_counters: [0] searches, [1] zero-lambda results, [2] reruns because the k-NN a-posteriori check failed,
    // [3] reruns because a candidate buffer overflowed, [4] reruns because the scorer's check failed, [5] searches that
    // took at least one rerun (under qmu)
    mutable int64_t scount[6] = {0, 0, 0, 0, 0, 0};
    // as_sweep_counters: [0] as_search_taus calls, [1] shared passes that served at least one tau, [2] tau values a shared
    // pass did not serve (or could not be run for) that were redone by the single search
    mutable std::atomic<int64_t> sweep_count[3] = {};
    // as_batch_sweep_counters: [0] as_search_batch_taus calls, [1] batched passes whose scorer tail served a tau sweep, [2] (query,
    // tau) pairs such a pass served, [3] pairs it left to the single search
    mutable std::atomic<int64_t> bsweep_count[4] = {};
    // as_subset_sweep_counters: [0] tau sweeps over a subset (all four forms), [1] score-kernel launches they made, [2] tau planes
    // those launches wrote, [3] lambda_q steps run (single searches plus as_search_batch calls)
    mutable std::atomic<int64_t> ssweep_count[4] = {};
    // as_score_items: the score kernel's buffers (as_subset.hip), made on first use and grown on demand; calls are serialised (smu)
    mutable struct as::SubsetWork* score_ws = nullptr;
    mutable std::mutex smu;
    // as_score_lists_batch / as_search_lists_batch: their buffers (as_lists.hip), made on first use and grown on demand; calls
    // are serialised (lmu).  as_lists_counters: [0] calls, [1] score-kernel launches, [2] (query, item) pairs scored, [3] lambda_q
    // steps run, [4] host nanoseconds spent on id checks, deduplication and work tables
    mutable struct as::ListsWork* lists_ws = nullptr;
    mutable std::mutex lmu;
    mutable std::atomic<int64_t> lists_count[5] = {};
    // as_lists_sweep_counters (the _taus forms; same buffers, same mutex): [0] calls, [1] score-kernel launches, [2] (query, item)
    // pairs gathered, once per launch, [3] (query, item, tau) scores written, [4] lambda_q steps run, [5] host nanoseconds as
    // lists_count[4]
    mutable std::atomic<int64_t> lsweep_count[6] = {};
    mutable int64_t unproven_searches = 0;   // searches returned although their a-posteriori check failed on the strongest path
    mutable double kstats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // accumulated by as_knn_rows
    // as_search_range / as_search_range_batch with sub == NULL: a subset of all items (no host id list: position == id), made on
    // first use under rmu and kept (4 bytes per item on the device, plus the score buffer of the route); calls are serialised by
    // its mutex.  as_range_counters: [0] calls that passed their checks, [1] compaction launches, [2] scores examined, [3]
    // survivors returned, [4] compaction relaunches after the append buffer overflowed, [5] lambda_q steps run.  range_us: the
    // compaction kernel of the last call under "range_timing" (as_range_kernel_us)
    mutable as_subset* range_all = nullptr;
    mutable std::mutex rmu;
    mutable std::atomic<int64_t> range_count[6] = {};
    mutable std::atomic<double> range_us{0.0};
    // as_search_fused / as_score_fused: the search form runs on the caller's subset or on range_all, the
    // score form on score_ws (under smu).  as_fused_counters: [0] calls that passed their checks, [1] accumulate launches, [2]
    // scores folded (served rows x m), [3] lambda_q steps run.  fused_us: the accumulate kernel of the last call under
    // "fused_timing" (as_fused_kernel_us)
    mutable std::atomic<int64_t> fused_count[4] = {};
    mutable std::atomic<double> fused_us{0.0};
    // as_search_fused_batch / as_score_fused_batch: on the same buffers as the single forms.
    // as_fused_batch_counters: [0] calls that passed their checks, [1] needs of those calls, [2] accumulate launches, [3] scores
    // folded (served rows x m), [4] lambda_q steps run (1 per call), [5] need groups begun.  fused_batch_us: the accumulate kernel
    // of the last call under "fused_batch_timing" (as_fused_batch_kernel_us)
    mutable std::atomic<int64_t> fused_batch_count[6] = {};
    mutable std::atomic<double> fused_batch_us{0.0};
    // as_search_grouped / as_search_grouped_batch: they run on the caller's subset or on range_all.
    // as_grouped_counters: [0] calls that passed their checks, [1] pick-kernel launches, [2] scores examined (rows x m per pick
    // launch), [3] 64-bit max-atomics the pick kernels issued, [4] groups returned, [5] members returned, [6] lambda_q steps run.
    // grouped_us: the pick kernels of the last call under "grouped_timing" (as_grouped_kernel_us)
    mutable std::atomic<int64_t> grouped_count[7] = {};
    mutable std::atomic<double> grouped_us{0.0};
    // as_search_maxsim / as_score_maxsim: they run on the caller's subset or on range_all.
    // as_maxsim_counters: [0] calls that passed their checks, [1] vectors served, [2] pass-A launches, [3] 64-bit max-atomics
    // pass A issued, [4] fold launches.  maxsim_us: pass A (with the memset of its cells) and the fold kernel of the last call
    // under "maxsim_timing" (as_maxsim_kernel_us)
    mutable std::atomic<int64_t> maxsim_count[5] = {};
    mutable std::atomic<double> maxsim_us[2] = {};
    // as_search_maxsim_batch / as_score_maxsim_batch: on the same buffers as the single forms.
    // as_maxsim_batch_counters: [0] calls that passed their checks, [1] needs of those calls, [2] vectors served, [3] pass-A
    // launches, [4] 64-bit max-atomics pass A issued, [5] fold launches, [6] lambda_q steps run (1 per call), [7] need groups
    // begun.  maxsim_batch_us: pass A (with the memset of its cells) and the segmented fold kernel of the last call under
    // "maxsim_batch_timing" (as_maxsim_batch_kernel_us)
    mutable std::atomic<int64_t> maxsim_batch_count[8] = {};
    mutable std::atomic<double> maxsim_batch_us[2] = {};
    // as_search_maxsim_lists / as_score_maxsim_lists: their buffers (as_maxsim_lists.hip), made on
    // first use and grown on demand; calls are serialised by lmu, the per-query list forms' mutex.  as_maxsim_lists_counters: [0]
    // calls that passed their checks, [1] needs of those calls, [2] vectors served, [3] score-kernel launches, [4] rows the score
    // kernel was asked to gather (entries x vector tiles), [5] (vector, row) dots, [6] fold launches, [7] lambda_q steps run (1
    // per call), [8] host nanoseconds spent on the checks and the work tables.  maxsim_lists_us: the score kernel, the fold
    // kernel and the selection (or the copy out) of the last call under "maxsim_lists_timing" (as_maxsim_lists_kernel_us)
    mutable struct as::MaxsimListsWork* mlists_ws = nullptr;
    mutable std::atomic<int64_t> maxsim_lists_count[9] = {};
    mutable std::atomic<double> maxsim_lists_us[3] = {};
    // as_search_diverse / as_search_diverse_batch: their buffers (as_diverse.hip), made on first use and grown on demand; the
    // selection step of a call is serialised by dmu (the pool step before it is an ordinary search and takes no lock of these).
    // as_diverse_counters: [0] calls that passed their checks, [1] select launches, [2] picks made, [3] dots computed, [4] pool
    // steps run (ordinary searches, single or batched)
    mutable struct as::DiverseWork* diverse_ws = nullptr;
    mutable std::mutex dmu;
    mutable std::atomic<int64_t> diverse_count[5] = {};
    // as_search_diffuse / as_search_diffuse_batch / as_score_diffuse_batch / as_diffuse_seeds: their
    // buffers (as_diffuse.hip), made on first use and grown on demand; the recurrence of a call is serialised by fmu (the pool step
    // before it is an ordinary search and takes no lock of these; the search forms take fmu INSIDE the mutex of the handle whose
    // selection buffers they use, always in that order, and nothing takes a handle's mutex under fmu).  as_diffuse_counters: [0]
    // calls that passed their checks, [1] route searches run (single or batched), [2] column chunks, [3] step launches, [4] seeds
    // uploaded
    mutable struct as::DiffuseWork* diffuse_ws = nullptr;
    mutable std::mutex fmu;
    mutable std::atomic<int64_t> diffuse_count[5] = {};
    // the solve forms share diffuse_ws and fmu.  as_diffuse_solve_counters: [0] calls that passed their
    // checks, [1] route searches run, [2] column chunks, [3] iterations launched, [4] host waits, [5] seeds uploaded
    mutable std::atomic<int64_t> diffuse_solve_count[6] = {};
    // as_graph_eigs shares diffuse_ws and fmu.  as_graph_eigs_counters: [0] calls that passed their
    // checks, [1] outer iterations, [2] step launches, [3] Gram launches, [4] rotate launches, [5] host waits
    mutable std::atomic<int64_t> eigs_count[6] = {};
    // as_graph_components / as_graph_components_sweep share diffuse_ws and fmu.
    // as_components_counters: [0] calls that passed their checks, [1] thresholds served (1 for a call without one), [2] hook
    // launches, [3] compress launches, [4] host waits
    mutable std::atomic<int64_t> components_count[5] = {};
};

struct as_graph {
    int device = 0;
    int64_t n = 0;
    int64_t nnz = 0;          // adjacency entries (both directions, no diagonal)
    as_graph_params gp{};     // sigma resolved
    int metric = 0, kernel = 0;
    int64_t* indptr = nullptr;  // [n+1]
    int32_t* indices = nullptr; // [nnz] ascending per row
    double* dist = nullptr;     // [nnz] d_ij
    double* gy = nullptr;       // [nnz] y_i . y_j
    double* w = nullptr;        // [nnz] a_ij
    double* lap = nullptr;      // [nnz] -a_ij / sqrt(deg_i deg_j)
    double* deg = nullptr;      // [n]
    double* ny = nullptr;       // [n] |y_i|^2
    double* E = nullptr;        // [n]
    double* G = nullptr;        // [n]
    double tau0 = 0.0;
    double stats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // feature mode (AS_LAMBDA_FEATURE): n == nfeatures, the CSR above is the feature graph (lap = -w, the
    // off-diagonal of L = D - W), nitems the number of items E / G / the lambdas cover
    int lambda_mode = 0;
    int64_t nitems = 0;
    int64_t e_rows = 0;         // feature mode: entries E / G hold -- nitems after as_feat_lambdas_global (every item's, all-gathered),
                                // the space's own rows after a single-space build or a load
    int64_t ne = 0;             // edges a < b
    int32_t* ea = nullptr;      // [ne]
    int32_t* eb = nullptr;
    double* ew = nullptr;
    double* colm = nullptr;     // [n] squared column norms (the Gram's diagonal)
    // row-sharded item graph (as_graph_shard_*): the CSR holds the rows [row0, row0 + n) of the graph over ncols
    // items, column ids global; deg / ny / E / G cover these rows only.  ncols == 0: a whole graph (ncols = n).
    int64_t ncols = 0;
    int64_t row0 = 0;
};
inline int64_t graph_items(const as_graph* gr) {   // items the index covers
    return gr->lambda_mode == AS_LAMBDA_FEATURE ? gr->nitems : (gr->ncols ? gr->ncols : gr->n);
}

// a set of items of one space (as_subset_create): sorted unique ids, on the host and in the work buffers
struct as_subset {
    const as_space* sp = nullptr;
    int64_t m = 0;
    int64_t* ids = nullptr;      // [m] host copy (as_subset_ids); null in the space's own subset of all items (position == id)
    as::SubsetWork* w = nullptr;
    mutable std::mutex mu;       // calls on one handle are serialised
};

// the groups of the items of one space (as_groups_create): every item's dense group number, groups numbered by ascending label
struct as_groups {
    const as_space* sp = nullptr;
    int device = 0;
    int64_t n = 0, count = 0;        // items, distinct labels
    std::vector<int32_t> dense;      // [n] item -> group
    std::vector<int64_t> labels;     // [count] group -> the caller's label, ascending
    std::vector<int32_t> size;       // [count] items of the group
    int32_t* dense_dev = nullptr;    // [n] the same on the device, uploaded once
};

// the answer of a range query (as_search_range, as_search_range_batch): host memory only, independent of the space
struct as_range {
    int64_t nq = 0;                // lists
    bool count_only = false;       // offsets only
    std::vector<int64_t> offs;     // [nq + 1]
    std::vector<int64_t> idx;      // [offs[nq]] item ids, each list by (score descending, id ascending)
    std::vector<double> score;
};

// ---------------------------------------------------------------- device helpers
#if defined(__HIPCC__)
namespace as {

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// LDS hand-off between lanes of ONE wave: the hardware keeps a wave's LDS operations in
// order; wait for them and stop the compiler from caching LDS values across the point.
#define AS_LDS_FENCE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// Scratch device allocation of a host function: freed on every return path, error paths included.
template <typename T>
struct dev_tmp {
    T* p = nullptr;
    dev_tmp() = default;
    dev_tmp(const dev_tmp&) = delete;
    dev_tmp& operator=(const dev_tmp&) = delete;
    ~dev_tmp() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t count) { return hipMalloc((void**)&p, sizeof(T) * (count ? count : 1)); }
    operator T*() const { return p; }
};

// Grow-only work buffers of a handle, in device memory (dev_buf) and in pinned host memory (pin_buf): freed with their owner.
// reserve(count): nothing if `count` elements fit already; else the old block is freed and exactly `count` elements are
// allocated (the contents are lost; the caller pads `count` if it wants room to grow).  After a failure the buffer is empty.
struct dev_mem {
    static hipError_t get(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void put(void* p) { (void)hipFree(p); }
};
struct pin_mem {
    static hipError_t get(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void put(void* p) { (void)hipHostFree(p); }
};
template <typename T, typename Mem>
class work_buf {
    T* p = nullptr;
    size_t n = 0;

public:
    work_buf() = default;
    work_buf(const work_buf&) = delete;
    work_buf& operator=(const work_buf&) = delete;
    ~work_buf() { release(); }
    hipError_t reserve(size_t count) {
        if (count <= n) return hipSuccess;
        release();
        const hipError_t e = Mem::get((void**)&p, sizeof(T) * count);
        if (e == hipSuccess) n = count;
        else p = nullptr;
        return e;
    }
    void release() {
        if (p) Mem::put(p);
        p = nullptr;
        n = 0;
    }
    size_t size() const { return n; }
    operator T*() const { return p; }
};
template <typename T>
using dev_buf = work_buf<T, dev_mem>;
template <typename T>
using pin_buf = work_buf<T, pin_mem>;

// reserve() as a status: a failure names the part and the size asked for
template <typename B>
as_status reserve_or_err(B& buf, int64_t count, const char* part) {
    const hipError_t e = buf.reserve((size_t)count);
    if (e == hipSuccess) return AS_OK;
    set_err("allocation of the %s (%lld elements) failed: %s", part, (long long)count, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? AS_ENOMEM : AS_EHIP;
}

// HIP events of a host function: destroyed on every return path, error paths included.
template <int N>
struct dev_events {
    hipEvent_t e[N] = {};
    dev_events() = default;
    dev_events(const dev_events&) = delete;
    dev_events& operator=(const dev_events&) = delete;
    ~dev_events() {
        for (int i = 0; i < N; ++i)
            if (e[i]) (void)hipEventDestroy(e[i]);
    }
    hipError_t create() {
        for (int i = 0; i < N; ++i) {
            const hipError_t r = hipEventCreate(&e[i]);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    }
};

// SPEC S6 edge energy w ||y_i/sqrt(d_i) - y_j/sqrt(d_j)||^2 from the stored pair quantities; a value inside the rounding
// noise of the expanded form's terms is zero: a neighbour identical to the node must not become a 1e-16 "energy"
// whose share of the sum is 1
// (DESIGN.md section 2, S7).
// The form does not cancel for near-identical neighbours (alpha = d_i^-1/2, beta = d_j^-1/2):
//   l2:     alpha beta dist^2 + (alpha - beta)(alpha n_i - beta n_j)   (dist^2 summed as differences)
//   cosine: (alpha - beta)^2 + 2 alpha beta (1 - c) for unit vectors, alpha^2 n_i + beta^2 n_j if one is zero
__host__ __device__ __forceinline__ double edge_energy(double w, int metric, double dist, double g, double di, double dj,
                                                        double nyi, double nyj) {
    const double alpha = 1.0 / sqrt(di), beta = 1.0 / sqrt(dj);
    double core;
    if (metric == AS_METRIC_L2) core = alpha * beta * (dist * dist) + (alpha - beta) * (alpha * nyi - beta * nyj);
    else if (nyi > 0.0 && nyj > 0.0) core = (alpha - beta) * (alpha - beta) + 2.0 * alpha * beta * (1.0 - g);
    else core = alpha * alpha * nyi + beta * beta * nyj;
    const double v = w * core;
    const double floor_ = w * 0x1p-46 * (alpha * alpha * nyi + beta * beta * nyj + 2.0 * alpha * beta * fabs(g));
    return v > floor_ ? v : 0.0;
}
// SPEC S2 cosine distance: rounding can push a cosine past 1 -- no negative distances (a fractional p would turn
// them into NaN weights)
__host__ __device__ __forceinline__ double cosine_distance(double c) { return 1.0 - (c > 0.0 ? (c < 1.0 ? c : 1.0) : 0.0); }

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float bcast_lane(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}
__device__ __forceinline__ int bcast_lane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ double bcast_lane(double v, int src) {
    long long b = __double_as_longlong(v);
    int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), src);
    int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

template <typename T>
__device__ __forceinline__ bool lex_less(T ka, int ia, T kb, int ib) {
    return ka < kb || (ka == kb && ia < ib);
}

template <typename T>
struct key_traits;
template <>
struct key_traits<float> {
    static __device__ __forceinline__ float inf() { return __int_as_float(0x7f800000); }
};
template <>
struct key_traits<double> {
    static __device__ __forceinline__ double inf() { return __longlong_as_double(0x7ff0000000000000LL); }
};

// Wave-resident sorted candidate list ("wavefront-shuffle top-k"): lane t holds
// the t-th smallest (key, idx) seen so far; slots >= m stay (+inf, INT_MAX).
template <typename T>
struct WaveList {
    T key;
    int idx;
    __device__ __forceinline__ void init() {
        key = key_traits<T>::inf();
        idx = 0x7fffffff;
    }
    // threshold = entry m-1
    __device__ __forceinline__ void thr(int m, T& tk, int& ti) const {
        tk = bcast_lane(key, m - 1);
        ti = bcast_lane(idx, m - 1);
    }
    // insert a wave-uniform candidate; caller guarantees (ck,ci) < entry m-1
    __device__ __forceinline__ void insert(T ck, int ci) {
        const int lane = lane_id();
        const bool less = lex_less<T>(key, idx, ck, ci);
        const int pos = __popcll(__ballot(less));
        T pk = __shfl_up(key, 1, 64);
        int pi = __shfl_up(idx, 1, 64);
        if (lane == pos) {
            key = ck;
            idx = ci;
        } else if (lane > pos) {
            key = pk;
            idx = pi;
        }
    }
    // offer one candidate per lane (inactive lanes pass valid=false)
    __device__ __forceinline__ void offer(int m, T ck, int ci, bool valid) {
        T tk;
        int ti;
        thr(m, tk, ti);
        bool pass = valid && lex_less<T>(ck, ci, tk, ti);
        unsigned long long mask = __ballot(pass);
        while (mask) {
            const int src = __ffsll((long long)mask) - 1;
            const T bk = bcast_lane(ck, src);
            const int bi = bcast_lane(ci, src);
            if (lex_less<T>(bk, bi, tk, ti)) {
                insert(bk, bi);
                thr(m, tk, ti);
            }
            mask &= mask - 1;
            // drop lanes that no longer beat the tightened threshold
            pass = pass && lex_less<T>(ck, ci, tk, ti);
            mask &= __ballot(pass);
        }
    }
};

// 128-slot variant (k up to 120): slot t in (key, idx), slot 64 + t in (key2, idx2); same contract as WaveList.
template <typename T>
struct WaveList2 {
    T key, key2;
    int idx, idx2;
    __device__ __forceinline__ void init() {
        key = key2 = key_traits<T>::inf();
        idx = idx2 = 0x7fffffff;
    }
    __device__ __forceinline__ void thr(int m, T& tk, int& ti) const {
        if (m <= 64) {
            tk = bcast_lane(key, m - 1);
            ti = bcast_lane(idx, m - 1);
        } else {
            tk = bcast_lane(key2, m - 65);
            ti = bcast_lane(idx2, m - 65);
        }
    }
    __device__ __forceinline__ void insert(T ck, int ci) {
        const int lane = lane_id();
        const int pos = __popcll(__ballot(lex_less<T>(key, idx, ck, ci))) + __popcll(__ballot(lex_less<T>(key2, idx2, ck, ci)));
        const T pk = __shfl_up(key, 1, 64), pk2 = __shfl_up(key2, 1, 64);
        const int pi = __shfl_up(idx, 1, 64), pi2 = __shfl_up(idx2, 1, 64);
        const T lk = bcast_lane(key, 63);      // slot 63 moves up into slot 64
        const int li = bcast_lane(idx, 63);
        const int g2 = 64 + lane;
        if (g2 == pos) {
            key2 = ck;
            idx2 = ci;
        } else if (g2 > pos) {
            key2 = lane == 0 ? lk : pk2;
            idx2 = lane == 0 ? li : pi2;
        }
        if (lane == pos) {
            key = ck;
            idx = ci;
        } else if (lane > pos) {
            key = pk;
            idx = pi;
        }
    }
    __device__ __forceinline__ void offer(int m, T ck, int ci, bool valid) {
        T tk;
        int ti;
        thr(m, tk, ti);
        bool pass = valid && lex_less<T>(ck, ci, tk, ti);
        unsigned long long mask = __ballot(pass);
        while (mask) {
            const int src = __ffsll((long long)mask) - 1;
            const T bk = bcast_lane(ck, src);
            const int bi = bcast_lane(ci, src);
            if (lex_less<T>(bk, bi, tk, ti)) {
                insert(bk, bi);
                thr(m, tk, ti);
            }
            mask &= mask - 1;
            pass = pass && lex_less<T>(ck, ci, tk, ti);
            mask &= __ballot(pass);
        }
    }
};

// the blend of src/lib.rs:166-173 as SPEC S11 has it, from an exact cosine: ONE definition, so that every path that ranks
// exact scores (single GPU, staged, one-exchange, filtered) rounds alike
__device__ __forceinline__ double blend_score(double tau, double c, double lq, double lj) {
    return tau * c + (1.0 - tau) / (1.0 + fabs(lq - lj));
}

// Selection key of a scored entry (the filtered and the list searches): 96 bits hi:lo, hi = the score's bits mapped so that a
// larger score is a larger number (NaN lowest, -0 as +0), lo = the caller's tie-break.  Eight digits of 12 bits.
__device__ __forceinline__ unsigned long long sel_ord(double s) {
    if (s != s) return 0ull;
    if (s == 0.0) s = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(s);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
// digit p (0 = most significant) of the key hi:lo
__device__ __forceinline__ unsigned int sel_digit(unsigned long long hi, unsigned int lo, int p) {
    if (p <= 4) return (unsigned int)(hi >> (52 - 12 * p)) & 0xfffu;
    if (p == 5) return ((unsigned int)(hi & 0xfull) << 8) | (lo >> 24);
    return p == 6 ? (lo >> 12) & 0xfffu : lo & 0xfffu;
}
// the key agrees with t_hi:t_lo in its first p digits
__device__ __forceinline__ bool sel_match(unsigned long long hi, unsigned int lo, unsigned long long t_hi, unsigned int t_lo, int p) {
    const int nb = 12 * p;
    const unsigned long long mh = nb >= 64 ? ~0ull : (nb == 0 ? 0ull : ~0ull << (64 - nb));
    const unsigned int ml = nb <= 64 ? 0u : ~0u << (96 - nb);
    return ((hi ^ t_hi) & mh) == 0ull && ((lo ^ t_lo) & ml) == 0u;
}

// SPEC S4 edge weight.  gaussian: exp(-0.5 (d/sigma)^p); rational: 1/(1+(d/sigma)^p)
__device__ __forceinline__ double edge_weight(double d, double sigma, double p, int kernel) {
    const double t = d / sigma;
    const double u = (p == 2.0) ? t * t : pow(t, p);
    return kernel == AS_KERNEL_GAUSSIAN ? exp(-0.5 * u) : 1.0 / (1.0 + u);
}

}  // namespace as
#endif  // __HIPCC__

// ---------------------------------------------------------------- internal entry points
namespace as {

// |q|^2 exactly as q_prepare_kernel (as_search.hip) forms it on the device -- 256 strided partial sums, element c in partial
// c % 256, rounded products and sums, then the halving tree: the host-prepared fast path, the staged / batched paths and the
// filtered and list searches must give a query the same norm, bit for bit, so that their cosines share a denominator.  Whoever
// changes the order there changes it here.  (No fma on either side: std::fma without -mfma is a library call, 6 us for 768
// elements.)
inline double host_sumsq(const double* q, int64_t d) {
    double p[256];
    for (int t = 0; t < 256; ++t) p[t] = 0.0;
    for (int64_t c = 0; c < d; ++c) {     // element c belongs to partial c % 256, visited in increasing c: the kernel's order
        volatile double sq = q[c] * q[c];   // rounded product, kept apart from the sum (no contraction whatever the flags)
        p[c & 255] = p[c & 255] + sq;
    }
    for (int o = 128; o > 0; o >>= 1)
        for (int t = 0; t < o; ++t) p[t] += p[t + o];
    return p[0];
}

struct Scratch;  // growable device scratch owned by a call

as_status resolve_params(const as_graph_params* gp, as_graph_params* out);
as_status check_limits(const as_graph_params* resolved, int64_t n, int lambda_mode);
// per-pair fp32 error coefficient: |key32 - key64| <= coef * (n_i + n_j) for L2,
// <= coef for cosine
double err_coef(const as_space* sp);
as_status ring_i8_stats(as_space* sp, double* out3);
as_status ring_i8_set(as_space* sp, double u_max, double v_max, int32_t usable);
// the int8 two-digit image of the space's items (x8, fa8, u8max, v8max, coef8), made on first use; *present: it exists and
// holds no non-finite item (whether its error is acceptable is the caller's call: build pass, scan)
as_status space_i8_image(const as_space* sp, bool* present);
as_status space_i8h_image(const as_space* sp, bool* present);
as_status space_nib_image(const as_space* sp, bool* present);

// build stages (as_build.hip)
as_status ingest(as_space* sp, const void* items_dev, int dtype, int64_t ld);
as_status ingest_host(as_space* sp, const double* items, int64_t row_stride, int64_t col_stride);
as_status knn_rows(const as_space* sp, const as_graph_params* gp, int64_t r0, int64_t r1, int32_t* out_idx,
                   double* out_key, double* out_dist, double* out_gy, int32_t* out_cnt, double* stats);
as_status graph_from_knn(as_space* sp, const as_graph_params* gp, const int32_t* idx, const double* dist,
                         const double* gy, const int32_t* cnt, as_graph* gr);
as_status csr_from_knn(hipStream_t st, int64_t n, int64_t k, const int32_t* idx, const double* dist, const double* gy,
                       const int32_t* cnt, double sigma, double p, int kernel, as_graph* gr);
as_status median_lambda(as_space* sp, as_graph* gr, const double* E, const double* G);
as_status median_lambda_n(hipStream_t st, int64_t n, const double* E, const double* G, double* lam64, float* lam32, double* tau0_out);
as_status lam_slice(hipStream_t st, int64_t n, const double* src, double* lam64, float* lam32);
as_status graph_shard_csr(as_space* sp, const as_graph_params* gp, int64_t n_global, int64_t row_offset, const int32_t* idx,
                          const double* dist, const double* gy, const int32_t* cnt, int64_t n_in, const int32_t* in_row,
                          const int32_t* in_col, const double* in_dist, const double* in_gy, as_graph* gr);
as_status graph_shard_energy(as_space* sp, as_graph* gr, const double* deg_global, const double* n64_global);
as_status graph_shard_lambdas(as_space* sp, as_graph* gr, const double* E_global, int64_t n_global);
as_status graph_from_knn_global(as_space* sp, const as_graph_params* gp, int64_t n_global, int64_t row_offset, const int32_t* idx,
                                const double* dist, const double* gy, const int32_t* cnt, const double* n64_global, as_graph* gr);
// k-NN over visiting column blocks (multi-GPU ring, as_build.hip)
as_status knn_block(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t r0, int64_t r1, int64_t row_goff,
                    int64_t col_goff, int M, double* p_key, double* p_dist, double* p_gy, int32_t* p_idx, int32_t* p_cnt, float* p_t32);
as_status knn_merge(const as_space* sp, const as_graph_params* gp, int64_t r0, int64_t r1, int nblocks, int M, const double* p_key,
                    const double* p_dist, const double* p_gy, const int32_t* p_idx, const int32_t* p_cnt, const float* p_t32,
                    const double* block_nmax_host, int32_t* out_idx, double* out_key, double* out_dist, double* out_gy,
                    int32_t* out_cnt, int32_t* flag, double* out_B, int64_t* nflagged);
as_status knn_block_band(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t r0, int64_t r1, int64_t row_goff,
                         int64_t col_goff, int M, int32_t* flag, const double* B, double* p_key, double* p_dist, double* p_gy,
                         int32_t* p_idx, int32_t* p_cnt, float* p_t32, int64_t* overflowed);
int knn_list_width(int64_t k);
as_status knn_block_exact(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t r0, int64_t r1, int64_t row_goff,
                          int64_t col_goff, int M, const int32_t* flag, double* p_key, double* p_dist, double* p_gy, int32_t* p_idx,
                          int32_t* p_cnt, float* p_t32);
as_status knn_block_pair(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t r0, int64_t r1, int64_t ct0,
                         int64_t ct1, int64_t row_goff, int64_t col_goff, const float* col_thr, const float* row_thr, int M, double* p_key,
                         double* p_dist, double* p_gy, int32_t* p_idx, int32_t* p_cnt, float* p_t32, double* q_key, double* q_dist, double* q_gy,
                         int32_t* q_idx, int32_t* q_cnt, float* q_t32);
as_status knn_thresholds(const as_space* sp, int64_t r0, int64_t r1, int M, double nmax_all, const double* r_key, const int32_t* r_cnt,
                         float* out_thr);
as_status knn_fold(const as_space* sp, int64_t r0, int64_t r1, int M, int mode, double block_nmax, const int32_t* flag, double* r_key,
                   double* r_dist, double* r_gy, int32_t* r_idx, int32_t* r_cnt, float* r_t32, const double* b_key, const double* b_dist,
                   const double* b_gy, const int32_t* b_idx, const int32_t* b_cnt, const float* b_t32);

// feature mode (as_feat.hip)
as_status feat_gram(const as_space* sp, int64_t r0, int64_t r1, double* gram);
as_status feat_graph(const as_space* sp, const as_graph_params* gp, const double* gram, as_graph* gr);
as_status feat_energy(const as_space* sp, const as_graph* gr, int64_t r0, int64_t r1, double* E, double* G);
as_status feat_build(as_space* sp, const as_graph_params* gp, as_graph* gr);
as_status feat_edges_from_csr(as_graph* gr, hipStream_t st);   // rebuilds ea/eb/ew from the CSR (index load)
struct QInfo;
as_status feat_query_prepare(const as_graph* gr, const double* qin, int64_t d, int64_t dp, double* q64, float* q32, QInfo* info,
                             int nslots, hipStream_t st);

// query-as-row exact k-NN used by the build fallback (as_search.hip)
as_status exact_row_knn(as_query* ws, const as_graph_params* gp, int64_t row, int32_t* out_idx,
                        double* out_key, double* out_dist, double* out_gy, int32_t* out_cnt);
as_status search_once(as_query* q, const double* query, int64_t d, double tau, int exact, int64_t* out_idx,
                      double* out_score, int64_t* out_len, double* out_lambda_q);
as_status search_sweep(as_query* q, const double* query, int64_t d, const double* taus, int nt, int64_t lstride, int64_t* out_idx,
                       double* out_score, int64_t* out_len, double* out_lambda_q, int* served);
void query_flags(const as_query* q, int* knn_inexact, int* score_inexact);
int query_overflow_bits(const as_query* q);
as_status query_create(const as_space* sp, const as_graph* gr, int cap, as_query** out, int pool_slot = 0);
as_status search_batch_launch(as_query* q, const double* queries, int nb, int64_t d, double tau);
as_status search_batch_launch_pair(as_query* a, as_query* b, const double* qa, int nba, const double* qb, int nbb, int64_t d, double tau);
as_status search_batch_collect(as_query* q, int nb, double tau, int64_t topk, int64_t* out_idx, double* out_score, int64_t* out_len,
                               double* out_lambda_q, int32_t* out_status);
as_status search_batch_sweep_launch(as_query* q, const double* queries, int nb, int64_t d, const double* taus, int nt);
as_status search_batch_sweep_launch_pair(as_query* a, as_query* b, const double* qa, int nba, const double* qb, int nbb, int64_t d,
                                         const double* taus, int nt);
as_status search_batch_sweep_collect(as_query* q, int nb, const double* taus, int nt, int64_t topk, int64_t* out_idx, double* out_score,
                                     int64_t* out_len, double* out_lambda_q, int32_t* out_status);
int query_sweep_ran(const as_query* q);
// Small host steps the filtered, list and range searches share.
// The query stage of a chunk at dst: [nbp][dp] queries i0 .. i0 + nb - 1 of `queries` ([.][d]), zero padded (rows >= nb all
// zero), then [nbp] |q|^2 (host_sumsq), then [nbp] lambda_q.
inline void stage_queries(double* dst, const double* queries, int64_t i0, int64_t nb, int64_t nbp, int64_t d, int64_t dp, const double* lq) {
    double* hn = dst + nbp * dp;
    double* hl = hn + nbp;
    for (int64_t t = 0; t < nbp; ++t) {
        double* row = dst + t * dp;
        const int64_t dt = t < nb ? d : 0;   // (a pad row: zeros throughout)
        const double* q = queries + (i0 + (t < nb ? t : 0)) * d;
        for (int64_t c = 0; c < dt; ++c) row[c] = q[c];
        for (int64_t c = dt; c < dp; ++c) row[c] = 0.0;
        hn[t] = t < nb ? host_sumsq(q, d) : 0.0;
        hl[t] = t < nb ? lq[i0 + t] : 0.0;
    }
}
// fn(t, u) for every maximal run [t, u) of queries i0 + t, t < nb, whose status is not AS_EZEROLAMBDA: what a chunk holds for
// the others is no answer and is not copied out
template <typename F>
as_status for_served_runs(const int32_t* status, int64_t i0, int64_t nb, F&& fn) {
    for (int64_t t = 0; t < nb;) {
        if (status[i0 + t] == AS_EZEROLAMBDA) {
            ++t;
            continue;
        }
        int64_t u = t;
        while (u < nb && status[i0 + u] != AS_EZEROLAMBDA) ++u;
        AS_TRY(fn(t, u));
        t = u;
    }
    return AS_OK;
}
// waits for the stream; timing: *us += the time between the two events recorded on it
inline as_status sync_add_elapsed(hipStream_t stream, bool timing, const hipEvent_t* ev, double* us) {
    AS_HIP(hipStreamSynchronize(stream));
    if (timing) {
        float ms = 0.0f;
        AS_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        *us += (double)ms * 1e3;
    }
    return AS_OK;
}

// filtered search (as_subset.hip): exact S11 scores of a list of items gathered by id, exact top-k of them.  A SubsetWork holds
// everything a call needs on the device (ids, scores, the query, the selection's histograms and records) and the pinned result.
// ONE set of grow-only buffers serves the single-query, the batched and the tau-sweep forms (subset_reserve): created for a single
// query (nothing is allocated per single query), grown by the first larger call of another form, never shrunk.  One call at a
// time per SubsetWork (the owner's mutex).
constexpr int SUBSET_TOPK = 1024;   // == MAX_TOPK: entries of the final one-block sort
struct SubsetOut {
    int64_t len;
    int64_t idx[SUBSET_TOPK];
    double score[SUBSET_TOPK];
};
struct SubsetSel;
struct SubsetWork {
    int device = 0;
    hipStream_t stream = nullptr;
    int cus = 256;                 // compute units of that device (the score kernel's grid)
    int64_t cap = 0, dp = 0;       // ids the handle holds (< 2^31: positions are 32-bit), padded query length
    dev_buf<int32_t> ids;          // [cap]
    dev_buf<double> qd;            // the query stage (stage_queries): [rows][dp] queries, then [rows] |q|^2, then [rows] lambda_q
    pin_buf<double> qh;            // pinned staging of the same
    dev_buf<double> scores;        // at least [cap]; the batched forms: [chunk][m]; the sweeps: the [query][tau][m] planes of a (chunk, tau group)
    // the selection's scratch, per row (a query, or a (query, tau) pair of a sweep)
    dev_buf<unsigned int> hist;    // one histogram per radix pass, then the counter of selected positions
    dev_buf<SubsetSel> state;      // the threshold's digits found so far, per pass
    dev_buf<int32_t> sel_pos;      // [SUBSET_TOPK] positions at or above the threshold
    pin_buf<SubsetOut> out;        // pinned, written by the sort kernel
    hipEvent_t ev[2] = {nullptr, nullptr};
    int timing = 0;                // record ev around the score kernel
    double kernel_us = 0.0;        // ... and its duration in the last timed call (the batched forms: summed over the chunks)
    // range search (as_range.hip): the append buffer, its counters and the thresholds, made on the first range call on this work
    RangeWork* range = nullptr;
    // fused multi-query search (as_fused.hip): the accumulator, the weights and the flags, made on the first fused call on this work
    FusedWork* fused = nullptr;
    // grouped search (as_grouped.hip): the cells, the collapsed scores and the picks, made on the first grouped call on this work
    GroupedWork* grouped = nullptr;
    // late-interaction search (as_maxsim.hip): the cells, the accumulator, the weights and the flags, made on the first such call on this work
    MaxsimWork* maxsim = nullptr;
};
as_status subset_work_create(const as_space* sp, int64_t cap, SubsetWork** out);
void subset_work_free(SubsetWork* w);
as_status subset_set_ids(SubsetWork* w, const int32_t* ids_host, int64_t m);
as_status subset_score(const as_space* sp, SubsetWork* w, int64_t m, const double* query, double tau, double lambda_q);
as_status subset_select(SubsetWork* w, int64_t m, int64_t k, int64_t* out_idx, double* out_score, int64_t* out_len);
as_status subset_scores_out(SubsetWork* w, int64_t m, double* out);
// The batched forms over the m ids of `w`: b queries [b][d] with their lambda_q and status (AS_EZEROLAMBDA: no output for that
// query), in chunks of queries on the work's stream, one wait per chunk.  k > 0: the first k of every query's scores ->
// out_idx / out_score at stride `stride`, out_len; k == 0: all scores -> out_scores [b][m], or, with a sink, to the sink: it is
// called once per chunk behind the score kernel with the chunk's scores ([nb][ld], still on the device, queued on the work's
// stream; a zero-lambda query's row holds no answer); range search's sink waits for the stream itself, the fused forms' sink only
// queues its kernel: the run's one wait per chunk follows either way.
struct SubsetChunkSink {
    as_status (*fn)(void* ctx, SubsetWork* w, int64_t i0, int64_t nb, const double* scores, int64_t ld);
    void* ctx;
    int64_t row_bytes = 0;   // device bytes the sink keeps per query of a chunk beside the m scores: the chunk budget counts them
};
as_status subset_batch_run(const as_space* sp, SubsetWork* w, int64_t m, const double* queries, int64_t b, const double* lq,
                           const int32_t* status, double tau, int64_t k, int64_t stride, int64_t* out_idx, double* out_score,
                           int64_t* out_len, double* out_scores, const SubsetChunkSink* sink = nullptr);
void set_subset_batch_mib(int v);   // as_set_tuning("subset_batch_mib", v)
constexpr int64_t SB_QC_MAX = 4096;   // queries of a chunk at most: the rows the selection serves at once
// as_set_tuning("filtered_grid_cap", v): v > 0 clips gridDim.x of the filtered family's stride-loop kernels (the gather score
// kernels, the radix select's passes, the lists' segments, the fused and late-interaction folds, the grouped picks, the range compaction) to at most v
// blocks, so that tests drive the later trips of those loops at small shapes; 0 (the default): every grid is what its call site
// computes.  Results never depend on it.
void set_filtered_grid_cap(int v);
int64_t filtered_grid(int64_t blocks);   // the grid a call site computed, under the cap
// The selection over ONE row of m scores that lie anywhere on the device (the positions are those of the work's ids), queued on
// the work's stream behind whatever wrote them: the first k by (score descending, position ascending) -> ids and scores; waits for
// the stream.
as_status subset_select_from(SubsetWork* w, const double* scores, int64_t m, int64_t k, int64_t* out_idx, double* out_score, int64_t* out_len);
// ... with the position -> id table of the answer as an argument ([m] int32 on the device) in place of the work's ids: the same
// kernels over positions that are not items of the subset (late-interaction search: position == dense group number).
as_status subset_select_from_table(SubsetWork* w, const double* scores, const int32_t* pos_ids, int64_t m, int64_t k, int64_t* out_idx,
                                   double* out_score, int64_t* out_len);
// ... and over `rows` rows ([rows][ld]) at once, all under the one table pos_ids (the work's ids, or a caller's own): row t's list
// -> w->out[t] (len == min(k, m, SUBSET_TOPK)); waits for the stream.
as_status subset_select_rows_from(SubsetWork* w, const double* scores, const int32_t* pos_ids, int64_t ld, int64_t m, int64_t k, int64_t rows);
// a row's pinned result (w->out[row]) of k entries to the caller's arrays; AS_EHIP if the selection left another length there
as_status subset_list_out(const SubsetOut* o, int64_t k, int64_t* out_idx, double* out_score, int64_t* out_len);
constexpr int QUERY_BATCH = 32;  // == GQ in as_search.hip: query slots of the batched workspace
constexpr int TAU_GROUP = 8;     // taus one shared pass of a tau sweep serves (search_sweep, as_search_taus; one gather of a subset)
// Tau sweeps over the m ids of `w`: nt distinct finite taus, up to TAU_GROUP per gather.  The list / the
// scores of taus[u] go to row row[u] of the outputs: k > 0: out_idx / out_score + row * k, out_len[row]; k == 0: out_scores +
// row * m.  The batched form: rows i * ntau + row[u] for query i; status AS_EZEROLAMBDA: nothing is written for that query.
// counts[0] += score-kernel launches, counts[1] += tau planes they wrote.  One stream wait per (chunk, tau group).
as_status subset_sweep_run(const as_space* sp, SubsetWork* w, int64_t m, const double* query, double lambda_q, const double* taus, int64_t nt,
                           const int64_t* row, int64_t k, int64_t* out_idx, double* out_score, int64_t* out_len, double* out_scores,
                           int64_t* counts);
as_status subset_batch_sweep_run(const as_space* sp, SubsetWork* w, int64_t m, const double* queries, int64_t b, const double* lq,
                                 const int32_t* status, const double* taus, int64_t nt, const int64_t* row, int64_t ntau, int64_t k,
                                 int64_t* out_idx, double* out_score, int64_t* out_len, double* out_scores, int64_t* counts);
// Per-query candidate lists (as_lists.hip): list i = ids[offs[i] .. offs[i + 1]) (item ids, checked by the
// caller; the search form: distinct within a list) belongs to query i.  One ragged score launch per chunk of queries whose
// entries fit the "subset_batch_mib" budget.  kk > 0: the first min(kk, list length) of every list by (score descending, index
// ascending) -> out_idx / out_score + i * kk, out_len[i]; kk == 0: every score -> out_scores[offs[i] ..].  status
// AS_EZEROLAMBDA: nothing is scored or written for that query (out_len 0).  counts[0] += score-kernel launches, [1] += pairs
// scored, [2] += host nanoseconds spent on the work tables.  The buffers live in sp->lists_ws (under sp->lmu).
as_status lists_run(const as_space* sp, const int32_t* ids, const int64_t* offs, const double* queries, int64_t b, const double* lq,
                    const int32_t* status, double tau, int64_t kk, int64_t* out_idx, double* out_score, int64_t* out_len,
                    double* out_scores, int64_t* counts);
// The tau sweep over the same lists: nt distinct finite taus, up to TAU_GROUP per gather, one upload per
// chunk for all its groups; tau taus[u] goes to row row[u] of the ntau rows a query owns.  kk > 0: list (i, row) -> out_idx /
// out_score + (i * ntau + row) * kk, out_len[i * ntau + row]; kk == 0: out_scores[ntau * offs[i] + row * m_i + e].  counts[0] +=
// score-kernel launches, [1] += pairs gathered (once per launch), [2] += scores written, [3] += host nanoseconds on the tables.
as_status lists_run_taus(const as_space* sp, const int32_t* ids, const int64_t* offs, const double* queries, int64_t b, const double* lq,
                         const int32_t* status, const double* taus, int64_t nt, const int64_t* row, int64_t ntau, int64_t kk, int64_t* out_idx,
                         double* out_score, int64_t* out_len, double* out_scores, int64_t* counts);
void lists_work_free(ListsWork* w);
double lists_kernel_us(const ListsWork* w);
void set_lists_timing(int v);   // as_set_tuning("lists_timing", 0 | 1)
void set_lists_budget_mib(int v);   // as_set_tuning("subset_batch_mib", v): the value set_subset_batch_mib gets
int64_t lists_budget_doubles();     // ... as the scores (doubles) a chunk may hold
// lists_select_kernel over nb lists that lie anywhere on the device, queued on `stream`: list t = entries lists[2 t] ..
// lists[2 t] + lists[2 t + 1] - 1 of scores / ids (a length of 0: no answer); the first min(kk, length) entries by (score
// descending, id ascending; the ids of a list distinct) -> out_idx / out_score + t * kk, out_len[t] (pinned).  Does not wait.
as_status lists_select_launch(hipStream_t stream, const int64_t* lists, const double* scores, const int32_t* ids, int64_t kk, int64_t nb,
                              int64_t* out_len, int64_t* out_idx, double* out_score);
// Range search (as_range.hip): the survivors of nq rows of m scores ([nq][ld] on the device, queued on the
// work's stream) against one threshold per row (NaN: that row has no answer) are appended to `res` as nq further lists, each by
// (score descending, id ascending); ids_host maps a position to its id (null: position == id).  count_only: the lists' lengths
// alone.  Waits for the stream.  counts[0] += compaction launches, [1] += scores examined, [2] += survivors, [3] += relaunches
// after an overflow of the append buffer; *us += the compaction kernel's microseconds under "range_timing".
as_status range_compact(SubsetWork* w, const double* scores, int64_t ld, int64_t m, int64_t nq, const double* thr_host, bool count_only,
                        const int64_t* ids_host, as_range* res, int64_t* counts, double* us);
void range_work_free(RangeWork* r);
void set_range_cap(int v);      // as_set_tuning("range_cap", v)
void set_range_timing(int v);   // as_set_tuning("range_timing", 0 | 1)
// Fused multi-query search (as_fused.hip): the fold of j rows of scores over the work's m ids into one
// accumulator [m] on the device.  fused_begin: room for the call, its weights and served flags (status AS_EZEROLAMBDA: not
// served) uploaded once on the work's stream.  fused_chunk: rows i0 .. i0 + nb - 1 of the call, [nb][ld] on the device, folded
// onto the accumulator behind the kernel that wrote them -- the sink of subset_batch_run; it does not wait.  A chunk without a
// served row launches nothing.  fused_end: after the caller's last wait for the stream.  mode 0: sum, 1: max (S13).
struct FusedCall {
    SubsetWork* w = nullptr;
    int64_t m = 0;
    int mode = 0;
    bool fresh = true;             // no served row folded yet: the next launch initialises the accumulator
    bool timing = false, timed = false;
    int64_t launches = 0, folded = 0;   // accumulate launches, scores folded (served rows x m)
    double us = 0.0;               // the accumulate kernel's microseconds under "fused_timing"
};
as_status fused_begin(SubsetWork* w, int64_t m, int64_t j, const double* weights, const int32_t* status, int mode, FusedCall* c);
as_status fused_chunk(FusedCall* c, int64_t i0, int64_t nb, const double* scores, int64_t ld);
as_status fused_end(FusedCall* c);
const double* fused_acc(const SubsetWork* w);   // [m], valid after a call with a served row
void fused_work_free(FusedWork* f);
void set_fused_timing(int v);   // as_set_tuning("fused_timing", 0 | 1)
// The batched form: b needs, need y = the flattened rows offs[y] .. offs[y + 1] - 1 of the call's nv
// vectors, each folded into an accumulator row of its own.  fused_batch_begin: G = gmax needs per group from the "fused_batch_mib"
// budget (1 <= G <= SB_QC_MAX), room for [G][m] accumulators, ONE upload of the weights, the segment offsets, every need's first
// and last served row and the served flags (weights, status: [nv]).  fused_batch_group: needs g0 .. g0 + gn - 1 are in flight,
// need g0 + t owns accumulator row t.  fused_batch_chunk: rows i0 .. i0 + nb - 1 of THAT GROUP's slice of the vectors, [nb][ld]
// on the device -- the sink of a subset_batch_run over the slice; it does not wait; a chunk without a served row launches
// nothing.  fused_batch_end: after the caller's last wait for the stream.  The rows are fused_acc(w) + t * m.
// The parameters of a call over b needs of nv flattened vectors, in the pinned block and on the device, in the order of the one
// upload (the batched fused forms and batched late-interaction search): [nv] weights, [b + 1] int64 offsets, [b] int64 first and
// [b] int64 last served flattened row of every need (-1: none), [nv] int32 served flags.
struct BatchPar {
    double* wts;
    int64_t* offs;
    int64_t* first;
    int64_t* last;
    int32_t* flags;
    BatchPar(double* base, int64_t nv, int64_t b)
        : wts(base), offs((int64_t*)(base + nv)), first(offs + b + 1), last(first + b), flags((int32_t*)(last + b)) {}
    static int64_t words(int64_t nv, int64_t b) { return nv + (b + 1) + 2 * b + (nv + 1) / 2; }
    static size_t bytes(int64_t nv, int64_t b) { return sizeof(double) * (size_t)(nv + (b + 1) + 2 * b) + sizeof(int32_t) * (size_t)nv; }
    // filled from the caller's offsets, weights and per-vector status (AS_EZEROLAMBDA: not served); returns the served vectors
    int64_t fill(int64_t b, const int64_t* o, const double* weights, const int32_t* status) const {
        int64_t served = 0;
        for (int64_t y = 0; y <= b; ++y) offs[y] = o[y];
        for (int64_t y = 0; y < b; ++y) {
            first[y] = last[y] = -1;
            for (int64_t t = o[y]; t < o[y + 1]; ++t) {
                wts[t] = weights[t];
                flags[t] = status[t] == AS_EZEROLAMBDA ? 0 : 1;
                if (flags[t]) {
                    if (first[y] < 0) first[y] = t;
                    last[y] = t;
                    ++served;
                }
            }
        }
        return served;
    }
};
struct FusedBatchCall {
    SubsetWork* w = nullptr;
    int64_t m = 0, b = 0, nv = 0;
    int mode = 0;
    int64_t gmax = 1;              // G
    int64_t g0 = 0, gn = 0;        // the group in flight
    bool timing = false, timed = false;
    int64_t launches = 0, folded = 0, groups = 0;   // accumulate launches, scores folded (served rows x m), groups begun
    double us = 0.0;               // the accumulate kernel's microseconds under "fused_batch_timing"
};
as_status fused_batch_begin(SubsetWork* w, int64_t m, int64_t b, const int64_t* offs, const double* weights, const int32_t* status, int mode,
                            FusedBatchCall* c);
void fused_batch_group(FusedBatchCall* c, int64_t g0, int64_t gn);
as_status fused_batch_chunk(FusedBatchCall* c, int64_t i0, int64_t nb, const double* scores, int64_t ld);
as_status fused_batch_end(FusedBatchCall* c);
void set_fused_batch_timing(int v);   // as_set_tuning("fused_batch_timing", 0 | 1)
void set_fused_batch_mib(int v);      // as_set_tuning("fused_batch_mib", v): v > 0 MiB, v < 0 -v KiB, 0 the default (256 MiB)
// Grouped search (as_grouped.hip): the S14 answer of `rows` rows of scores over the work's m ids
// ([rows][ld] on the device, queued on the work's stream): row t belongs to query i0 + t of the call.  Query i's groups -> out_label /
// out_count + i * n_groups, their members -> out_idx / out_score + (i * n_groups + s) * per_group, out_ngroups[i].  status (null: the
// single form) AS_EZEROLAMBDA: that query gets 0 groups.  Two waits for the stream (one when no selected group has a second
// member to give).  counts[0] += pick launches, [1] += scores examined, [2] += max-atomics issued, [3] += groups, [4] += members;
// us += the pick kernels' microseconds under "grouped_timing".
constexpr int GROUPED_MAX_PER_GROUP = 16;
struct GroupedCall {
    SubsetWork* w = nullptr;
    const as_groups* g = nullptr;
    int64_t m = 0, n_groups = 0, per_group = 0;
    const int32_t* status = nullptr;
    int64_t* out_label = nullptr;
    int64_t* out_count = nullptr;
    int64_t* out_idx = nullptr;
    double* out_score = nullptr;
    int64_t* out_ngroups = nullptr;
    int64_t counts[5] = {0, 0, 0, 0, 0};
    double us = 0.0;
};
as_status grouped_rows(GroupedCall* c, int64_t i0, int64_t rows, const double* scores, int64_t ld);
int64_t grouped_row_bytes(const as_groups* g, int64_t m, int64_t n_groups, int64_t per_group);   // SubsetChunkSink::row_bytes of a call
void grouped_work_free(GroupedWork* g);
void set_grouped_timing(int v);   // as_set_tuning("grouped_timing", 0 | 1)
// pass A of round 0 of the pick kernel alone (as_grouped.hip): cells[row][g] <- the largest sel_ord key of group g in row `row` of
// scores ([rows][ld]) over the work's m ids, 0 where the group has no member; the caller zeroes the cells first; *natom += the
// global 64-bit max-atomics issued.  Queued on the work's stream; does not wait.
as_status group_max_launch(SubsetWork* w, const as_groups* gs, const double* scores, int64_t ld, int64_t m, int64_t rows,
                           unsigned long long* cells, unsigned long long* natom);
// Late-interaction search (as_maxsim.hip): F(g) = the S13 sum over the served vectors j, ascending, of
// w_j x the largest score of group g's members under vector j, folded into an accumulator [G] on the device (G = gs->count).
// maxsim_begin: room for the call, ONE upload of the weights and served flags (status AS_EZEROLAMBDA: not served).  maxsim_chunk:
// rows i0 .. i0 + nb - 1 of the call, [nb][ld] on the device -- the sink of subset_batch_run (row_bytes = 8 G); per run of served
// rows one memset of the cells and one pass-A launch, then ONE fold launch for the chunk; it does not wait; a chunk without a
// served row launches nothing.  maxsim_select: the first k groups by (F descending, group number ascending) -> group numbers and
// scores; waits.  maxsim_scores: the accumulator to out [G]; waits.  Both leave the counters and times of the call in *c.
struct MaxsimCall {
    SubsetWork* w = nullptr;
    const as_groups* g = nullptr;
    int64_t m = 0;
    bool fresh = true;             // no served row folded yet: the next fold launch initialises the accumulator
    bool timing = false, timed = false;
    int64_t served = 0, passa = 0, atoms = 0, folds = 0;   // vectors served, pass-A launches, max-atomics issued, fold launches
    double us[2] = {0.0, 0.0};     // pass A (with its memsets), the fold kernel: microseconds under "maxsim_timing"
};
as_status maxsim_begin(SubsetWork* w, const as_groups* gs, int64_t m, int64_t j, const double* weights, const int32_t* status, MaxsimCall* c);
as_status maxsim_chunk(MaxsimCall* c, int64_t i0, int64_t nb, const double* scores, int64_t ld);
as_status maxsim_select(MaxsimCall* c, int64_t k, int64_t* out_group, double* out_score, int64_t* out_len);
as_status maxsim_scores(MaxsimCall* c, double* out);
void maxsim_work_free(MaxsimWork* x);
void set_maxsim_timing(int v);   // as_set_tuning("maxsim_timing", 0 | 1)
// The batched form: b needs, need y = the flattened rows offs[y] .. offs[y + 1] - 1 of the call's nv
// vectors, each folded into an accumulator row [G] of its own.  maxsim_batch_begin: Gn = gmax needs per group from the
// "maxsim_batch_mib" budget (1 <= Gn <= SB_QC_MAX), room for [Gn][G] accumulators, ONE upload (BatchPar).  maxsim_batch_labels
// (the score form, once per call): the nl dense group numbers of the listed labels uploaded, room for [Gn][nl] listed scores.
// maxsim_batch_group: needs g0 .. g0 + gn - 1 are in flight, need g0 + t owns accumulator row t.  maxsim_batch_chunk: rows
// i0 .. i0 + nb - 1 of THAT GROUP's slice of the vectors, [nb][ld] on the device -- the sink of a subset_batch_run over the slice
// (row_bytes = 8 G): one memset of the cells, pass A per run of served rows, ONE segmented fold launch; it does not wait; a chunk
// without a served row launches nothing.  maxsim_batch_select: the first k groups of every need of the group in flight by (F
// descending, group number ascending) -> w->out[t]; waits.  maxsim_batch_pick: the listed F of the group's needs -> out
// [gn][nl], queued.  maxsim_batch_end: waits, leaves the atomics counted and the times in *c.
struct MaxsimBatchCall {
    SubsetWork* w = nullptr;
    const as_groups* g = nullptr;
    int64_t m = 0, b = 0, nv = 0, nl = 0;
    int64_t gmax = 1;              // Gn
    int64_t g0 = 0, gn = 0;        // the group in flight
    bool timing = false, timed = false;
    int64_t served = 0, passa = 0, atoms = 0, folds = 0, groups = 0;   // vectors served, pass-A launches, max-atomics, fold launches, groups begun
    double us[2] = {0.0, 0.0};     // pass A (with its memsets), the fold kernel: microseconds under "maxsim_batch_timing"
};
as_status maxsim_batch_begin(SubsetWork* w, const as_groups* gs, int64_t m, int64_t b, const int64_t* offs, const double* weights,
                             const int32_t* status, MaxsimBatchCall* c);
as_status maxsim_batch_labels(MaxsimBatchCall* c, const int32_t* gnum_host, int64_t nl);
void maxsim_batch_group(MaxsimBatchCall* c, int64_t g0, int64_t gn);
as_status maxsim_batch_chunk(MaxsimBatchCall* c, int64_t i0, int64_t nb, const double* scores, int64_t ld);
as_status maxsim_batch_select(MaxsimBatchCall* c, int64_t k);
as_status maxsim_batch_pick(MaxsimBatchCall* c, double* out);
as_status maxsim_batch_end(MaxsimBatchCall* c);
void set_maxsim_batch_timing(int v);   // as_set_tuning("maxsim_batch_timing", 0 | 1)
void set_maxsim_batch_mib(int v);      // as_set_tuning("maxsim_batch_mib", v): v > 0 MiB, v < 0 -v KiB, 0 the default (256 MiB)
// Late-interaction re-ranking of per-need candidate documents (as_maxsim_lists.hip).  The call as
// the entry points have checked and narrowed it: b needs, need y = the flattened vectors voffs[y] .. voffs[y + 1] - 1 with their
// lambda_q, status (AS_EZEROLAMBDA: not served) and weights, nst[y] != 0: the need is not served; need y's documents are
// need_docs[y] .. need_docs[y + 1] - 1, document dd = the entries doc_first[dd] .. doc_first[dd + 1] - 1 of ids (its members) and
// the dense group number doc_gnum[dd] (ascending inside a need).  kk > 0: need y's first min(kk, documents with a non-NaN F)
// documents by (F descending, group number ascending) -> out_gnum / out_score + y * kk, out_len[y]; kk == 0: F of every document
// -> out_F[dd] (NaN: a need that is not served, a document whose scores are all NaN).  Chunks of needs whose scores fit the
// "subset_batch_mib" budget, one stream wait each.  counts[0] += vectors served, [1] += score launches, [2] += rows asked for, [3]
// += dots, [4] += fold launches, [5] += host nanoseconds on the work tables; us[0..2]: the score kernel, the fold kernel, the
// selection or copy of this call under "maxsim_lists_timing".  The buffers live in sp->mlists_ws (under sp->lmu).
struct MaxsimListsIn {
    const double* queries = nullptr;   // [nv][d]
    const int64_t* voffs = nullptr;    // [b + 1]
    int64_t b = 0;
    const double* lq = nullptr;        // [nv]
    const int32_t* vst = nullptr;      // [nv]
    const int32_t* nst = nullptr;      // [b]
    const double* wts = nullptr;       // [nv]
    const int64_t* need_docs = nullptr;   // [b + 1]
    const int64_t* doc_first = nullptr;   // [nd + 1]
    const int32_t* doc_gnum = nullptr;    // [nd]
    const int32_t* ids = nullptr;         // [doc_first[nd]]
    double tau = 0.0;
    int64_t kk = 0;
};
as_status maxsim_lists_run(const as_space* sp, const MaxsimListsIn& in, int64_t* out_gnum, double* out_score, int64_t* out_len, double* out_F,
                           int64_t* counts, double* us);
void maxsim_lists_work_free(MaxsimListsWork* w);
int64_t maxsim_lists_tile(int64_t dp);   // vectors a tile of the score kernel holds at padded row length dp
int64_t maxsim_lists_segment();          // entries a segment holds at most
void set_maxsim_lists_timing(int v);     // as_set_tuning("maxsim_lists_timing", 0 | 1)
// Diversified search (as_diverse.hip): the greedy of S12 over b pools -- pool i = pool_idx / pool_score + i * kk,
// pool_len[i] <= kk entries in the order the route returned them (0: a query that is not served) -- n picks wanted, diversity delta.
// Pick t of query i -> out_idx / out_score / out_margin (may be null) + i * nn + t, nn = min(n, kk); out_len[i] = min(n, pool_len[i]).
// The ids and scores handed out are the pool's own (the kernel returns positions).  Chunks of "diverse_chunk" queries: one upload,
// one launch, one download, one stream wait each.  counts[0] += launches, [1] += picks, [2] += dots.  The buffers live in
// sp->diverse_ws (under sp->dmu).
as_status diverse_run(const as_space* sp, const int64_t* pool_idx, const double* pool_score, const int64_t* pool_len, int64_t kk, int64_t b,
                      int64_t n, double delta, int64_t* out_idx, double* out_score, double* out_margin, int64_t* out_len, int64_t* counts);
void diverse_work_free(DiverseWork* w);
double diverse_kernel_us(const DiverseWork* w);
void set_diverse_timing(int v);   // as_set_tuning("diverse_timing", 0 | 1)
void set_diverse_chunk(int v);    // as_set_tuning("diverse_chunk", v)
// Graph diffusion (as_diffuse.hip): the S19 recurrence for b queries over the whole graph `gr`.  Query
// i's seeds are the entries offs[i] .. offs[i + 1] - 1 of ids / vals (distinct ids inside [0, n), finite values: the caller has
// checked them); served (may be null) 0: that query is left out -- no column, no output.  Column chunks of C = 1, 16 or 64 queries
// ("diffuse_cols", "diffuse_mib"); per chunk one upload of the seed table, `steps` step launches (each followed by the seed
// kernel) on one stream, then the output:
//   sel != null: the first k of every served query's f over the m positions of pos_ids ([m] on the device: sel's ids) by (f
//     descending, position ascending) -> out_idx / out_score + i * stride, out_len[i] (the selection runs on sel's stream);
//   else pick_ids != null (host, [m]): f at those ids -> out_rows + i * m;
//   else the whole f -> out_rows + i * n.
// counts[0] += chunks, [1] += step launches, [2] += seeds uploaded.  The buffers live in sp->diffuse_ws (under sp->fmu).
struct DiffuseCall {
    int64_t b = 0;
    const int64_t* offs = nullptr;
    const int64_t* ids = nullptr;
    const double* vals = nullptr;
    const int32_t* served = nullptr;
    double alpha = 0.0;
    int64_t steps = 0;
    SubsetWork* sel = nullptr;
    const int32_t* pos_ids = nullptr;
    int64_t m = 0, k = 0, stride = 0;
    int64_t* out_idx = nullptr;
    double* out_score = nullptr;
    int64_t* out_len = nullptr;
    const int32_t* pick_ids = nullptr;
    double* out_rows = nullptr;
    // max_iters > 0: the S20 solve of the fixed point (as_diffuse_solve.hip) in place of `steps` steps; per query (each may be
    // null) the iterations run, sqrt(rho_last / bb) and 1 converged / 0 stopped at max_iters / 2 breakdown.  counts then holds
    // four: [0] += chunks, [1] += iterations launched, [2] += host waits, [3] += seeds uploaded
    double tol = 0.0;
    int64_t max_iters = 0;
    int32_t* out_iters = nullptr;
    double* out_residual = nullptr;
    int32_t* out_state = nullptr;
};
as_status diffuse_run(const as_space* sp, const as_graph* gr, const DiffuseCall& c, int64_t* counts);
void diffuse_work_free(DiffuseWork* w);
double diffuse_kernel_us(const DiffuseWork* w);
void set_diffuse_timing(int v);       // as_set_tuning("diffuse_timing", 0 | 1)
void set_diffuse_mib(int v);          // as_set_tuning("diffuse_mib", v): the byte budget of the two f buffers; 0: the default (1024 MiB)
void set_diffuse_cols(int v);         // as_set_tuning("diffuse_cols", v): columns of a chunk at most (1, 16 or 64); 0: the default (64)
void set_diffuse_tile_edges(int v);   // as_set_tuning("diffuse_tile_edges", v): edges of an LDS tile of the C = 1 kernel; 0: the default
void set_diffuse_grid_cap(int v);     // as_set_tuning("diffuse_grid_cap", v): v > 0 clips the step kernels' grids; results never depend on it
// the S20 solve (as_diffuse_solve.hip) runs through diffuse_run with c.max_iters > 0, on the same work buffers
double diffuse_solve_kernel_us(const DiffuseWork* w, int part);
void set_diffuse_solve_mib(int v);    // as_set_tuning("diffuse_solve_mib", v): the byte budget of the solve's four vectors; 0: the default (2048 MiB)
// Graph eigenpairs (as_spectral.hip): the m largest eigenvalues of S = -lap and their eigenvectors, on
// the diffusion forms' work buffers (under sp->fmu), the caller has checked every argument.  out_values [m] descending, out_vectors
// [m][n], out_residuals [m], out_info: [0] outer iterations, [1] 1 converged / 0 stopped at max_iters / 2 breakdown (the three
// arrays are then not written), [2] step launches, [3] C.  counts[0] += outer iterations, [1] += step launches, [2] += Gram
// launches, [3] += rotate launches, [4] += host waits.
struct SpectralCall {
    int m = 0, C = 0;
    double tol = 0.0;
    int64_t max_iters = 0;
    int degree = 0;
    int64_t seed = 0;
    double* out_values = nullptr;
    double* out_vectors = nullptr;
    double* out_residuals = nullptr;
    int64_t* out_info = nullptr;
};
as_status spectral_eigs(const as_space* sp, const as_graph* gr, const SpectralCall& c, int64_t* counts);
// one primitive on host blocks (as_spectral_op): n rows (the step: gr's), C = 16 or 64
as_status spectral_op(const as_space* sp, const as_graph* gr, int op, int64_t n, int C, const double* a_host, const double* b_host,
                      const double* t_host, const double* coef, double* out_host);
int sym_eig_host(const double* a, int n, double* w, double* v);
double spectral_kernel_us(const DiffuseWork* w, int part);
int64_t spectral_budget();            // "spectral_mib" in bytes
void set_spectral_mib(int v);         // as_set_tuning("spectral_mib", v): the byte budget of the eigensolver's four blocks; 0: the default (8192 MiB)
// Connected components (as_components.hip) of the whole graph `gr`, on the diffusion forms' workspace
// (under sp->fmu), the caller has checked every argument.  ts == null: every stored entry is kept, one stage, info [1]; else nt
// thresholds (none a NaN), info [nt] in the caller's order: the distinct ones run ascending, each from the last one's labels.
// labels_host (may be null): the [n] labels of the (last) stage.  counts[0] += hook launches, [1] += compress launches, [2] += host waits.
as_status components_run(const as_space* sp, const as_graph* gr, const double* ts, int32_t nt, int32_t* labels_host, as_components_info* info,
                         int64_t* counts);
double components_kernel_us(const DiffuseWork* w, int part);

}  // namespace as
