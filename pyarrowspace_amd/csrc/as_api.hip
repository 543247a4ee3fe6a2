// C ABI glue (include/arrowspace_hip.h): argument validation with the reference shim's
// error behaviour (/root/reference/src/helpers.rs:24-76, src/lib.rs:100-120,140-159),
// handle lifetime, and the composition of the staged build / search entry points.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <limits>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "as_common.hpp"

namespace as {

static std::atomic<int> g_debug{0};

std::string& err_slot() {
    static thread_local std::string s;
    return s;
}
void set_err(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err_slot() = buf;
}
bool debug_enabled() { return g_debug.load(std::memory_order_relaxed) != 0; }
void dbg(const char* fmt, ...) {
    if (!debug_enabled()) return;
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    fprintf(stderr, "[pyarrowspace] %s\n", buf);  // src/helpers.rs:18-20
}

static inline double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

as_status resolve_params(const as_graph_params* gp, as_graph_params* out) {
    if (!gp) {
        set_err("graph_params is required");
        return AS_EINVAL;
    }
    *out = *gp;
    if (!gp->has_sigma) out->sigma = gp->eps * 0.5;  // src/helpers.rs:68-72
    out->has_sigma = 1;
    if (!(out->eps > 0.0) || !(out->sigma > 0.0) || !(out->p > 0.0)) {
        set_err("graph_params: eps, sigma and p must be positive (eps=%g sigma=%g p=%g)", out->eps, out->sigma, out->p);
        return AS_EINVAL;
    }
    if (out->k < 1 || out->topk < 1) {
        set_err("graph_params: k and topk must be >= 1 (k=%lld topk=%lld)", (long long)out->k, (long long)out->topk);
        return AS_EINVAL;
    }
    return AS_OK;
}

// Hard limits of the selection kernels, checked before any upload or GPU work (the reference takes any usize,
// src/helpers.rs:56-63; INTEGRATION.md lists the caps): k-NN candidate lists are one slot per lane of a wave
// or two (k + 8 <= 128), scorer lists live in LDS (topk <= 1024).  Both are capped by the number of items first.
as_status check_limits(const as_graph_params* r, int64_t n, int lambda_mode) {
    const int64_t k = std::min<int64_t>(r->k, std::max<int64_t>(n - 1, 1));
    const int64_t topk = std::min<int64_t>(r->topk, n);
    if (k > 120 && lambda_mode != AS_LAMBDA_FEATURE) {   // the feature graph ranks whole columns: any k up to D - 1
        set_err("graph_params['k']=%lld exceeds the supported maximum of 120 for n=%lld", (long long)r->k, (long long)n);
        return AS_EUNSUPPORTED;
    }
    if (topk > 1024) {
        set_err("graph_params['topk']=%lld exceeds the supported maximum of 1024", (long long)r->topk);
        return AS_EUNSUPPORTED;
    }
    return AS_OK;
}

static as_status pick_device(const as_opts* opts, int* dev) {
    int d = opts ? opts->device : -1;
    if (d < 0) AS_HIP(hipGetDevice(&d));
    AS_HIP(hipSetDevice(d));
    *dev = d;
    return AS_OK;
}

// The pass pipeline of the batched searches (as_search_batch, batch_sweep_run; under sp->bmu, b > 1 queries on the workspaces of
// batch_workspaces).  A UNIT = the passes launched together: a pair (two workspaces), or one pass; two sets of workspaces
// alternate when there is more than one unit and the workspaces exist (`piped`): unit j + 1 is queued before unit j is waited for.
// launch(w0, i0, nb0, w1, i1, nb1): queue the pass of queries [i0, i0 + nb0) on w0 -- w1 set: with that of [i1, i1 + nb1) on w1,
// as a pair; collect(w, i0, nb): wait for the pass of queries [i0, i0 + nb) on w and hand out its results.
template <typename Launch, typename Collect>
static as_status batch_passes(const as_space* sp, int unit, int64_t b, Launch launch, Collect collect) {
    as_query* ws[4] = {sp->qcache_b, sp->qcache_b2, sp->qcache_b3, sp->qcache_b4};
    const bool piped = b > unit * QUERY_BATCH && ws[2 * unit - 1] != nullptr;
    const int nws = unit * (piped ? 2 : 1);
    // an error leaves no pass in flight behind it (the other workspaces' kernels would otherwise still be running when the
    // caller comes back)
    auto drain = [&](as_status s) {
        if (nws > 1)
            for (int w = 0; w < nws; ++w) (void)hipStreamSynchronize((hipStream_t)as_query_stream(ws[w]));
        return s;
    };
    const int64_t UNIT = (int64_t)unit * QUERY_BATCH;
    auto launch_unit = [&](int64_t j) -> as_status {
        as_query* const* w = ws + (piped ? unit * (j & 1) : 0);
        const int64_t i0 = j * UNIT, i1 = i0 + QUERY_BATCH;
        const bool pair = unit == 2 && i1 < b;
        return launch(w[0], i0, (int)std::min<int64_t>(QUERY_BATCH, b - i0), pair ? w[1] : nullptr, i1, pair ? (int)std::min<int64_t>(QUERY_BATCH, b - i1) : 0);
    };
    if (piped) {
        const as_status s0 = launch_unit(0);
        if (s0 != AS_OK) return drain(s0);
    }
    int64_t pass = 0;
    for (int64_t i0 = 0; i0 < b; i0 += QUERY_BATCH, ++pass) {
        const int64_t j = pass / unit;
        as_status s = AS_OK;
        if (pass % unit == 0) {   // a unit's first pass: queue the next unit (piped), or this one
            if (!piped) s = launch_unit(j);
            else if ((j + 1) * UNIT < b) s = launch_unit(j + 1);
        }
        if (s == AS_OK) s = collect(ws[(piped ? unit * (j & 1) : 0) + (int)(pass % unit)], i0, (int)std::min<int64_t>(QUERY_BATCH, b - i0));
        if (s != AS_OK) return drain(s);
    }
    return AS_OK;
}

}  // namespace as

using namespace as;

extern "C" {

void as_set_debug(int32_t enabled) { g_debug.store(enabled ? 1 : 0, std::memory_order_relaxed); }
const char* as_last_error(void) { return err_slot().c_str(); }
const char* as_version(void) { return "arrowspace-hip 0.1.0 (gfx950)"; }
int32_t as_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void as_free_space(as_space* sp) {
    if (!sp) return;
    hipSetDevice(sp->device);
    for (int i = 0; i < as_space::QPOOL; ++i)
        if (sp->qpool[i]) as_query_free(sp->qpool[i]);
    if (sp->qcache_b) as_query_free(sp->qcache_b);
    if (sp->qcache_b2) as_query_free(sp->qcache_b2);
    if (sp->qcache_b3) as_query_free(sp->qcache_b3);
    if (sp->qcache_b4) as_query_free(sp->qcache_b4);
    subset_work_free(sp->score_ws);
    as_subset_free(sp->range_all);
    lists_work_free(sp->lists_ws);
    maxsim_lists_work_free(sp->mlists_ws);
    diverse_work_free(sp->diverse_ws);
    diffuse_work_free(sp->diffuse_ws);
    if (sp->stream) hipStreamSynchronize(sp->stream);
    hipFree(sp->x32); hipFree(sp->xs); hipFree(sp->x8); hipFree(sp->x8h); hipFree(sp->x4); hipFree(sp->fa4); hipFree(sp->fa8); hipFree(sp->x64); hipFree(sp->n64); hipFree(sp->n32); hipFree(sp->inorm32);
    hipFree(sp->lam64); hipFree(sp->lam32);
    if (sp->stream) hipStreamDestroy(sp->stream);
    delete sp;
}

void as_free_graph(as_graph* gr) {
    if (!gr) return;
    hipSetDevice(gr->device);
    hipFree(gr->indptr); hipFree(gr->indices); hipFree(gr->dist); hipFree(gr->gy); hipFree(gr->w); hipFree(gr->lap);
    hipFree(gr->deg); hipFree(gr->ny); hipFree(gr->E); hipFree(gr->G);
    hipFree(gr->ea); hipFree(gr->eb); hipFree(gr->ew); hipFree(gr->colm);
    delete gr;
}

// a space without items yet: validated options, device, private stream
static as_status space_new(int64_t n, int64_t d, const as_opts* opts, as_space** out) {
    if (n >= (int64_t)1 << 31) {
        set_err("as_space_create_dev: n=%lld does not fit 32-bit item indices on one device", (long long)n);
        return AS_EUNSUPPORTED;
    }
    int dev = 0;
    AS_TRY(pick_device(opts, &dev));
    as_space* sp = new as_space();
    sp->device = dev;
    sp->n = n;
    sp->d = d;
    if (opts) sp->opts = *opts;
    sp->opts.device = dev;
    if (sp->opts.metric != AS_METRIC_L2 && sp->opts.metric != AS_METRIC_COSINE) {
        set_err("unknown metric %d", sp->opts.metric);
        delete sp;
        return AS_EINVAL;
    }
    if (sp->opts.kernel != AS_KERNEL_GAUSSIAN && sp->opts.kernel != AS_KERNEL_RATIONAL) {
        set_err("unknown kernel %d", sp->opts.kernel);
        delete sp;
        return AS_EINVAL;
    }
    if (sp->opts.lambda_mode != AS_LAMBDA_ITEM && sp->opts.lambda_mode != AS_LAMBDA_FEATURE) {
        set_err("unknown lambda_mode %d", sp->opts.lambda_mode);
        delete sp;
        return AS_EINVAL;
    }
    hipError_t e = hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_err("hipStreamCreate failed: %s", hipGetErrorString(e));
        delete sp;
        return AS_EHIP;
    }
    *out = sp;
    return AS_OK;
}

as_status as_space_create_dev(const void* items_dev, int32_t dtype, int64_t n, int64_t d, int64_t ld, const as_opts* opts,
                              as_space** out_space) {
    if (!out_space) {
        set_err("as_space_create_dev: null output");
        return AS_EINVAL;
    }
    *out_space = nullptr;
    if (!items_dev || n <= 0 || d <= 0) {
        set_err("items must be non-empty 2D array");  // src/helpers.rs:27-29
        return AS_EINVAL;
    }
    if (ld < d || (dtype != AS_DTYPE_F32 && dtype != AS_DTYPE_F64)) {
        set_err("as_space_create_dev: bad leading dimension or dtype");
        return AS_EINVAL;
    }
    as_space* sp = nullptr;
    AS_TRY(space_new(n, d, opts, &sp));
    // the items come from the caller's own stream(s), which a raw pointer does not name: everything queued on the
    // device has to be finished before the ingest (on the space's private non-blocking stream) reads them
    if (hipDeviceSynchronize() != hipSuccess) {
        set_err("as_space_create_dev: %s", hipGetErrorString(hipGetLastError()));
        as_free_space(sp);
        return AS_EHIP;
    }
    as_status s = ingest(sp, items_dev, dtype, ld);
    if (s != AS_OK) {
        as_free_space(sp);
        return s;
    }
    *out_space = sp;
    return AS_OK;
}

as_status as_knn_rows(const as_space* sp, const as_graph_params* gp, int64_t row_begin, int64_t row_end, int32_t* out_idx_dev,
                      double* out_key_dev, double* out_dist_dev, double* out_gy_dev, int32_t* out_cnt_dev) {
    if (!sp || !out_idx_dev || !out_key_dev || !out_dist_dev || !out_gy_dev || !out_cnt_dev) {
        set_err("as_knn_rows: null argument");
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    AS_HIP(hipSetDevice(sp->device));
    return knn_rows(sp, &r, row_begin, row_end, out_idx_dev, out_key_dev, out_dist_dev, out_gy_dev, out_cnt_dev, sp->kstats);
}

as_status as_graph_from_knn(as_space* sp, const as_graph_params* gp, const int32_t* idx_dev, const double* dist_dev,
                            const double* gy_dev, const int32_t* cnt_dev, as_graph** out_graph) {
    if (!sp || !idx_dev || !dist_dev || !gy_dev || !cnt_dev || !out_graph) {
        set_err("as_graph_from_knn: null argument");
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    AS_HIP(hipSetDevice(sp->device));
    as_graph* gr = new as_graph();
    const double t0 = now_s();
    as_status s = graph_from_knn(sp, &r, idx_dev, dist_dev, gy_dev, cnt_dev, gr);
    if (s != AS_OK) {
        as_free_graph(gr);
        return s;
    }
    for (int i = 0; i < 10; ++i) gr->stats[i] = sp->kstats[i];  // k-NN stage of this rank's rows
    gr->stats[4] = now_s() - t0;
    *out_graph = gr;
    return AS_OK;
}

as_status as_graph_from_knn_global(as_space* sp, const as_graph_params* gp, int64_t n_global, int64_t row_offset, const int32_t* idx_dev,
                                   const double* dist_dev, const double* gy_dev, const int32_t* cnt_dev, const double* n64_global_dev,
                                   as_graph** out_graph) {
    if (!sp || !idx_dev || !dist_dev || !gy_dev || !cnt_dev || !n64_global_dev || !out_graph) {
        set_err("as_graph_from_knn_global: null argument");
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    AS_HIP(hipSetDevice(sp->device));
    as_graph* gr = new as_graph();
    const double t0 = now_s();
    as_status s = graph_from_knn_global(sp, &r, n_global, row_offset, idx_dev, dist_dev, gy_dev, cnt_dev, n64_global_dev, gr);
    if (s != AS_OK) {
        as_free_graph(gr);
        return s;
    }
    for (int i = 0; i < 10; ++i) gr->stats[i] = sp->kstats[i];
    gr->stats[4] = now_s() - t0;
    *out_graph = gr;
    return AS_OK;
}

as_status as_graph_shard_csr(as_space* sp, const as_graph_params* gp, int64_t n_global, int64_t row_offset, const int32_t* idx_dev,
                             const double* dist_dev, const double* gy_dev, const int32_t* cnt_dev, int64_t n_in, const int32_t* in_row_dev,
                             const int32_t* in_col_dev, const double* in_dist_dev, const double* in_gy_dev, as_graph** out_graph) {
    if (!sp || !idx_dev || !dist_dev || !gy_dev || !cnt_dev || !out_graph || (n_in > 0 && (!in_row_dev || !in_col_dev || !in_dist_dev || !in_gy_dev))) {
        set_err("as_graph_shard_csr: null argument");
        return AS_EINVAL;
    }
    if (sp->opts.lambda_mode == AS_LAMBDA_FEATURE) {
        set_err("as_graph_shard_csr: the space was created for the feature-mode lambda");
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    AS_HIP(hipSetDevice(sp->device));
    as_graph* gr = new as_graph();
    const double t0 = now_s();
    as_status s = graph_shard_csr(sp, &r, n_global, row_offset, idx_dev, dist_dev, gy_dev, cnt_dev, n_in, in_row_dev, in_col_dev, in_dist_dev,
                                  in_gy_dev, gr);
    if (s != AS_OK) {
        as_free_graph(gr);
        return s;
    }
    for (int i = 0; i < 10; ++i) gr->stats[i] = sp->kstats[i];
    gr->stats[4] = now_s() - t0;
    *out_graph = gr;
    return AS_OK;
}
static as_status graph_rows_copy(const as_graph* gr, const double* src, double* out_dev, const char* who) {
    if (!gr || !src || !out_dev) {
        set_err("%s: null argument or the stage that fills it has not run", who);
        return AS_EINVAL;
    }
    AS_HIP(hipSetDevice(gr->device));
    // a device-to-device hipMemcpy returns before the copy has run (legacy default stream), and the caller's streams
    // are non-blocking: without the synchronisation its next kernel could read the destination too early
    AS_HIP(hipMemcpy(out_dev, src, sizeof(double) * gr->n, hipMemcpyDeviceToDevice));
    AS_HIP(hipDeviceSynchronize());
    return AS_OK;
}
as_status as_graph_deg_copy(const as_graph* gr, double* out_dev) { return graph_rows_copy(gr, gr ? gr->deg : nullptr, out_dev, "as_graph_deg_copy"); }
as_status as_graph_energy_copy(const as_graph* gr, double* out_dev) { return graph_rows_copy(gr, gr ? gr->E : nullptr, out_dev, "as_graph_energy_copy"); }
int64_t as_graph_row_offset(const as_graph* gr) { return gr ? gr->row0 : 0; }
int64_t as_graph_ncols(const as_graph* gr) { return gr ? (gr->ncols ? gr->ncols : gr->n) : 0; }
int64_t as_graph_nitems(const as_graph* gr) { return gr ? graph_items(gr) : 0; }
as_status as_graph_shard_energy(as_space* sp, as_graph* gr, const double* deg_global_dev, const double* n64_global_dev) {
    if (!sp || !gr || !deg_global_dev || !n64_global_dev || !gr->ncols || gr->n != sp->n) {
        set_err("as_graph_shard_energy: null argument or not the sharded graph of this space");
        return AS_EINVAL;
    }
    AS_HIP(hipSetDevice(sp->device));
    const double t0 = now_s();
    AS_TRY(graph_shard_energy(sp, gr, deg_global_dev, n64_global_dev));
    gr->stats[4] += now_s() - t0;
    return AS_OK;
}
as_status as_graph_shard_lambdas(as_space* sp, as_graph* gr, const double* E_global_dev, int64_t n_global) {
    if (!sp || !gr || !E_global_dev || !gr->ncols || gr->n != sp->n || !gr->E) {
        set_err("as_graph_shard_lambdas: null argument, not the sharded graph of this space, or as_graph_shard_energy has not run");
        return AS_EINVAL;
    }
    AS_HIP(hipSetDevice(sp->device));
    const double t0 = now_s();
    AS_TRY(graph_shard_lambdas(sp, gr, E_global_dev, n_global));
    gr->stats[4] += now_s() - t0;
    return AS_OK;
}

int32_t as_knn_list_width(int64_t k) { return knn_list_width(k); }
double as_space_nmax(const as_space* sp) { return sp ? sp->nmax : 0.0; }
int64_t as_unproven_searches(const as_space* sp) { return sp ? sp->unproven_searches : 0; }
as_status as_space_norms(const as_space* sp, double* out_dev) {
    if (!sp || !out_dev) {
        set_err("as_space_norms: null argument");
        return AS_EINVAL;
    }
    AS_HIP(hipSetDevice(sp->device));
    AS_HIP(hipMemcpy(out_dev, sp->n64, sizeof(double) * sp->n, hipMemcpyDeviceToDevice));
    AS_HIP(hipDeviceSynchronize());   // device-to-device: asynchronous to the host, and the caller's streams are non-blocking
    return AS_OK;
}
int64_t as_space_row_offset(const as_space* sp) { return sp ? sp->row_offset : 0; }

as_status as_ring_i8_stats(as_space* sp, double* out3) {
    if (!sp || !out3) {
        set_err("as_ring_i8_stats: null argument");
        return AS_EINVAL;
    }
    return ring_i8_stats(sp, out3);
}
as_status as_ring_i8_set(as_space* sp, double u_max, double v_max, int32_t usable) {
    if (!sp) {
        set_err("as_ring_i8_set: null argument");
        return AS_EINVAL;
    }
    return ring_i8_set(sp, u_max, v_max, usable);
}
int32_t as_ring_i8(const as_space* sp) { return sp ? sp->ring_i8 : 0; }

as_status as_knn_block(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t row_begin, int64_t row_end,
                       int64_t row_goff, int64_t col_goff, double* p_key_dev, double* p_dist_dev, double* p_gy_dev, int32_t* p_idx_dev,
                       int32_t* p_cnt_dev, float* p_t32_dev) {
    if (!sp || !cols || !p_key_dev || !p_dist_dev || !p_gy_dev || !p_idx_dev || !p_cnt_dev || !p_t32_dev) {
        set_err("as_knn_block: null argument");
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    const int M = knn_list_width(r.k);
    if (M < 0) {
        set_err("graph_params['k']=%lld exceeds the supported maximum of 120", (long long)r.k);
        return AS_EUNSUPPORTED;
    }
    AS_HIP(hipSetDevice(sp->device));
    const double t0 = now_s();
    const as_status s = knn_block(sp, cols, &r, row_begin, row_end, row_goff, col_goff, M, p_key_dev, p_dist_dev, p_gy_dev, p_idx_dev,
                                  p_cnt_dev, p_t32_dev);
    sp->kstats[1] += now_s() - t0;
    return s;
}

as_status as_knn_block_pair(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t row_begin, int64_t row_end,
                            int64_t col_tile_begin, int64_t col_tile_end, int64_t row_goff, int64_t col_goff, const float* col_thr_dev,
                            const float* row_thr_dev, double* p_key_dev, double* p_dist_dev, double* p_gy_dev, int32_t* p_idx_dev, int32_t* p_cnt_dev, float* p_t32_dev,
                            double* q_key_dev, double* q_dist_dev, double* q_gy_dev, int32_t* q_idx_dev, int32_t* q_cnt_dev, float* q_t32_dev) {
    if (!sp || !cols || !p_key_dev || !p_dist_dev || !p_gy_dev || !p_idx_dev || !p_cnt_dev || !p_t32_dev || !q_key_dev || !q_dist_dev ||
        !q_gy_dev || !q_idx_dev || !q_cnt_dev || !q_t32_dev) {
        set_err("as_knn_block_pair: null argument");
        return AS_EINVAL;
    }
    if (sp == cols) {
        set_err("as_knn_block_pair: a block is not paired with itself (as_knn_block)");
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    const int M = knn_list_width(r.k);
    if (M < 0) {
        set_err("graph_params['k']=%lld exceeds the supported maximum of 120", (long long)r.k);
        return AS_EUNSUPPORTED;
    }
    AS_HIP(hipSetDevice(sp->device));
    const double t0 = now_s();
    const as_status s = knn_block_pair(sp, cols, &r, row_begin, row_end, col_tile_begin, col_tile_end, row_goff, col_goff, col_thr_dev, row_thr_dev, M,
                                       p_key_dev, p_dist_dev, p_gy_dev, p_idx_dev, p_cnt_dev, p_t32_dev, q_key_dev, q_dist_dev, q_gy_dev,
                                       q_idx_dev, q_cnt_dev, q_t32_dev);
    sp->kstats[1] += now_s() - t0;
    return s;
}

as_status as_knn_thresholds(const as_space* sp, const as_graph_params* gp, int64_t row_begin, int64_t row_end, double nmax_all,
                            const double* r_key_dev, const int32_t* r_cnt_dev, float* out_thr_dev) {
    if (!sp || !r_key_dev || !r_cnt_dev || !out_thr_dev || row_begin < 0 || row_end > sp->n || row_begin > row_end) {
        set_err("as_knn_thresholds: null argument or bad row range");
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    const int M = knn_list_width(r.k);
    if (M < 0) {
        set_err("graph_params['k']=%lld exceeds the supported maximum of 120", (long long)r.k);
        return AS_EUNSUPPORTED;
    }
    AS_HIP(hipSetDevice(sp->device));
    return knn_thresholds(sp, row_begin, row_end, M, nmax_all, r_key_dev, r_cnt_dev, out_thr_dev);
}

as_status as_knn_merge(const as_space* sp, const as_graph_params* gp, int64_t row_begin, int64_t row_end, int32_t nblocks,
                       const double* p_key_dev, const double* p_dist_dev, const double* p_gy_dev, const int32_t* p_idx_dev,
                       const int32_t* p_cnt_dev, const float* p_t32_dev, const double* block_nmax_host, int32_t* out_idx_dev,
                       double* out_key_dev, double* out_dist_dev, double* out_gy_dev, int32_t* out_cnt_dev, int32_t* out_flag_dev,
                       double* out_band_dev, int64_t* out_nflagged) {
    if (!sp || !p_key_dev || !p_dist_dev || !p_gy_dev || !p_idx_dev || !p_cnt_dev || !p_t32_dev || !out_idx_dev ||
        !out_key_dev || !out_dist_dev || !out_gy_dev || !out_cnt_dev || !out_flag_dev || !out_band_dev || !out_nflagged || nblocks < 0 ||
        (nblocks > 0 && !block_nmax_host)) {
        set_err("as_knn_merge: null argument");
        return AS_EINVAL;
    }
    if (row_begin < 0 || row_end > sp->n || row_begin > row_end) {   // the kernel reads the rows' norms
        set_err("as_knn_merge: bad row range [%lld,%lld) for n=%lld", (long long)row_begin, (long long)row_end, (long long)sp->n);
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    if (knn_list_width(r.k) < 0) {
        set_err("graph_params['k']=%lld exceeds the supported maximum of 120", (long long)r.k);
        return AS_EUNSUPPORTED;
    }
    AS_HIP(hipSetDevice(sp->device));
    const double t0 = now_s();
    const as_status s = knn_merge(sp, &r, row_begin, row_end, nblocks, knn_list_width(r.k), p_key_dev, p_dist_dev, p_gy_dev, p_idx_dev,
                                  p_cnt_dev, p_t32_dev, block_nmax_host, out_idx_dev, out_key_dev, out_dist_dev, out_gy_dev, out_cnt_dev,
                                  out_flag_dev, out_band_dev, out_nflagged);
    sp->kstats[2] += now_s() - t0;
    return s;
}

as_status as_knn_fold(const as_space* sp, const as_graph_params* gp, int64_t row_begin, int64_t row_end, int32_t mode, double block_nmax,
                      const int32_t* flag_dev, double* r_key_dev, double* r_dist_dev, double* r_gy_dev, int32_t* r_idx_dev,
                      int32_t* r_cnt_dev, float* r_t32_dev, const double* b_key_dev, const double* b_dist_dev, const double* b_gy_dev,
                      const int32_t* b_idx_dev, const int32_t* b_cnt_dev, const float* b_t32_dev) {
    if (!sp || !r_key_dev || !r_dist_dev || !r_gy_dev || !r_idx_dev || !r_cnt_dev || !r_t32_dev || !b_key_dev || !b_dist_dev ||
        !b_gy_dev || !b_idx_dev || !b_cnt_dev || !b_t32_dev || (mode != 0 && !flag_dev) || mode < 0 || mode > 2) {
        set_err("as_knn_fold: null argument or bad mode");
        return AS_EINVAL;
    }
    if (row_begin < 0 || row_end > sp->n || row_begin > row_end) {   // the kernel reads the rows' norms
        set_err("as_knn_fold: bad row range [%lld,%lld) for n=%lld", (long long)row_begin, (long long)row_end, (long long)sp->n);
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    if (knn_list_width(r.k) < 0) {
        set_err("graph_params['k']=%lld exceeds the supported maximum of 120", (long long)r.k);
        return AS_EUNSUPPORTED;
    }
    AS_HIP(hipSetDevice(sp->device));
    return knn_fold(sp, row_begin, row_end, knn_list_width(r.k), mode, block_nmax, flag_dev, r_key_dev, r_dist_dev, r_gy_dev, r_idx_dev,
                    r_cnt_dev, r_t32_dev, b_key_dev, b_dist_dev, b_gy_dev, b_idx_dev, b_cnt_dev, b_t32_dev);
}

as_status as_knn_block_band(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t row_begin, int64_t row_end,
                            int64_t row_goff, int64_t col_goff, int32_t* flag_dev, const double* band_dev, double* p_key_dev,
                            double* p_dist_dev, double* p_gy_dev, int32_t* p_idx_dev, int32_t* p_cnt_dev, float* p_t32_dev,
                            int64_t* out_overflowed) {
    if (!sp || !cols || !flag_dev || !band_dev || !p_key_dev || !p_dist_dev || !p_gy_dev || !p_idx_dev || !p_cnt_dev || !p_t32_dev ||
        !out_overflowed) {
        set_err("as_knn_block_band: null argument");
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    AS_HIP(hipSetDevice(sp->device));
    const double t0 = now_s();
    const as_status s = knn_block_band(sp, cols, &r, row_begin, row_end, row_goff, col_goff, knn_list_width(r.k), flag_dev, band_dev,
                                       p_key_dev, p_dist_dev, p_gy_dev, p_idx_dev, p_cnt_dev, p_t32_dev, out_overflowed);
    sp->kstats[2] += now_s() - t0;
    if (s == AS_OK) sp->kstats[8] += (double)*out_overflowed;
    return s;
}

as_status as_knn_block_exact(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t row_begin, int64_t row_end,
                             int64_t row_goff, int64_t col_goff, const int32_t* flag_dev, double* p_key_dev, double* p_dist_dev,
                             double* p_gy_dev, int32_t* p_idx_dev, int32_t* p_cnt_dev, float* p_t32_dev) {
    if (!sp || !cols || !flag_dev || !p_key_dev || !p_dist_dev || !p_gy_dev || !p_idx_dev || !p_cnt_dev || !p_t32_dev) {
        set_err("as_knn_block_exact: null argument");
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    AS_HIP(hipSetDevice(sp->device));
    const double t0 = now_s();
    const as_status s = knn_block_exact(sp, cols, &r, row_begin, row_end, row_goff, col_goff, knn_list_width(r.k), flag_dev, p_key_dev,
                                        p_dist_dev, p_gy_dev, p_idx_dev, p_cnt_dev, p_t32_dev);
    sp->kstats[3] += now_s() - t0;
    return s;
}

// graph + Laplacian + lambdas over a space whose items are in place (t0: the call's start, t1: the end of the ingest)
static as_status build_from_space(as_space* sp, const as_graph_params& r, double t0, double t1, as_space** out_space, as_graph** out_graph) {
    const int64_t n = sp->n, d = sp->d;
    int32_t *idx = nullptr, *cnt = nullptr;
    double *key = nullptr, *dist = nullptr, *gy = nullptr;
    as_graph* gr = new as_graph();
    as_status s = AS_OK;
    if (sp->opts.lambda_mode == AS_LAMBDA_FEATURE) {
        // lambda on the F x F feature-space Laplacian: no N x N item graph at all
        s = feat_build(sp, &r, gr);
        if (s != AS_OK) {
            as_free_graph(gr);
            as_free_space(sp);
            return s;
        }
        gr->stats[0] = t1 - t0;
        gr->stats[5] = now_s() - t0;
        dbg("built ArrowSpace: nitems=%lld, nfeatures=%lld, lambdas_len=%lld", (long long)n, (long long)d, (long long)n);
        *out_space = sp;
        *out_graph = gr;
        return AS_OK;
    }
    do {
        hipError_t e;
        if ((e = hipMalloc(&idx, sizeof(int32_t) * n * r.k)) != hipSuccess || (e = hipMalloc(&cnt, sizeof(int32_t) * n)) != hipSuccess ||
            (e = hipMalloc(&key, sizeof(double) * n * r.k)) != hipSuccess || (e = hipMalloc(&dist, sizeof(double) * n * r.k)) != hipSuccess ||
            (e = hipMalloc(&gy, sizeof(double) * n * r.k)) != hipSuccess) {
            set_err("hipMalloc of the k-NN lists failed: %s", hipGetErrorString(e));
            s = AS_ENOMEM;
            break;
        }
        s = knn_rows(sp, &r, 0, n, idx, key, dist, gy, cnt, gr->stats);
        if (s != AS_OK) break;
        const double t2 = now_s();
        s = graph_from_knn(sp, &r, idx, dist, gy, cnt, gr);
        if (s != AS_OK) break;
        const double t3 = now_s();
        gr->stats[0] = t1 - t0;
        gr->stats[4] = t3 - t2;
        gr->stats[5] = t3 - t0;
    } while (0);
    hipFree(idx); hipFree(cnt); hipFree(key); hipFree(dist); hipFree(gy);
    if (s != AS_OK) {
        as_free_graph(gr);
        as_free_space(sp);
        return s;
    }
    dbg("built ArrowSpace: nitems=%lld, nfeatures=%lld, lambdas_len=%lld", (long long)n, (long long)d, (long long)n);
    *out_space = sp;
    *out_graph = gr;
    return AS_OK;
}

as_status as_build_dev(const void* items_dev, int32_t dtype, int64_t n, int64_t d, int64_t ld, const as_graph_params* gp,
                       const as_opts* opts, as_space** out_space, as_graph** out_graph) {
    if (!out_space || !out_graph) {
        set_err("as_build: null output");
        return AS_EINVAL;
    }
    *out_space = nullptr;
    *out_graph = nullptr;
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    if (n > 0) AS_TRY(check_limits(&r, n, opts ? opts->lambda_mode : 0));
    const double t0 = now_s();
    as_space* sp = nullptr;
    AS_TRY(as_space_create_dev(items_dev, dtype, n, d, ld, opts, &sp));
    return build_from_space(sp, r, t0, now_s(), out_space, out_graph);
}

// The reference's own call: float64 items in HOST memory, any numpy strides (/root/reference/src/lib.rs:271-277,
// src/helpers.rs:24-46 -- `as_array()` accepts them).  The rows stream to the device through two pinned chunks, the ingest
// kernel converting one chunk under the copy of the next (ingest_host): no device copy of the whole fp64 matrix.
as_status as_build(const double* items, int64_t n, int64_t d, int64_t row_stride, int64_t col_stride, const as_graph_params* gp,
                   const as_opts* opts, as_space** out_space, as_graph** out_graph) {
    if (!out_space || !out_graph) {
        set_err("as_build: null output");
        return AS_EINVAL;
    }
    *out_space = nullptr;
    *out_graph = nullptr;
    if (!items || n <= 0 || d <= 0) {
        set_err("items must be non-empty 2D array");  // src/helpers.rs:27-29
        return AS_EINVAL;
    }
    as_graph_params r;
    AS_TRY(resolve_params(gp, &r));
    AS_TRY(check_limits(&r, n, opts ? opts->lambda_mode : 0));   // before the upload
    dbg("items shape: (%lld, %lld)", (long long)n, (long long)d);  // src/helpers.rs:31
    const double t0 = now_s();
    as_space* sp = nullptr;
    AS_TRY(space_new(n, d, opts, &sp));
    const as_status s = ingest_host(sp, items, row_stride, col_stride);
    if (s != AS_OK) {
        as_free_space(sp);
        return s;
    }
    return build_from_space(sp, r, t0, now_s(), out_space, out_graph);
}

// ---------------------------------------------------------------- search
// ---- the pool of single-query workspaces (as_space::qpool).  pool_acquire hands out the lowest free slot -- a single
// thread always gets slot 0 --, grows the pool by one workspace when every existing one is busy (ARROWSPACE_SEARCH_POOL
// caps it, 1 .. QPOOL, default QPOOL) and otherwise waits for a release.  A search against ANOTHER graph handle waits for
// the pool to fall idle and rebuilds it (the workspaces carry the graph's k / topk layout).
static int pool_limit() {
    static const int lim = [] {
        const char* e = getenv("ARROWSPACE_SEARCH_POOL");
        const int v = e ? atoi(e) : as_space::QPOOL;
        return std::max(1, std::min(v, (int)as_space::QPOOL));
    }();
    return lim;
}

static as_status pool_acquire(const as_space* sp, const as_graph* gr, int* slot, as_query** out) {
    std::unique_lock<std::mutex> lk(sp->qmu);
    for (;;) {
        bool any = false, busy = false;
        for (int i = 0; i < as_space::QPOOL; ++i) {
            // (a slot reserved while its workspace is being made -- outside the lock -- belongs to qcache_gr like a finished one: a
            // caller with another graph handle must wait for it, not reserve a slot of its own beside it)
            any = any || sp->qpool[i] != nullptr || sp->qbusy[i];
            busy = busy || sp->qbusy[i];
        }
        if (any && sp->qcache_gr != gr) {
            if (busy) {
                sp->qcv.wait(lk);
                continue;
            }
            for (int i = 0; i < as_space::QPOOL; ++i) {
                if (sp->qpool[i]) as_query_free(sp->qpool[i]);
                sp->qpool[i] = nullptr;
            }
            sp->qcache = nullptr;
        }
        for (int i = 0; i < as_space::QPOOL; ++i)
            if (sp->qpool[i] && !sp->qbusy[i]) {
                sp->qbusy[i] = true;
                *slot = i;
                *out = sp->qpool[i];
                return AS_OK;
            }
        for (int i = 0; i < pool_limit(); ++i)
            if (!sp->qpool[i] && !sp->qbusy[i]) {
                sp->qbusy[i] = true;   // reserved while the workspace is being made (allocations: outside the lock)
                sp->qcache_gr = gr;
                lk.unlock();
                as_query* q = nullptr;
                const as_status s = query_create(sp, gr, 1, &q, i);
                lk.lock();
                if (s != AS_OK) {
                    sp->qbusy[i] = false;
                    sp->qcv.notify_all();
                    return s;
                }
                sp->qpool[i] = q;
                if (i == 0) sp->qcache = q;
                *slot = i;
                *out = q;
                return AS_OK;
            }
        sp->qcv.wait(lk);
    }
}

static void pool_release(const as_space* sp, int slot) {
    {
        std::lock_guard<std::mutex> lk(sp->qmu);
        sp->qbusy[slot] = false;
    }
    sp->qcv.notify_all();
}

static as_status search_single(const as_space* sp, const as_graph* gr, as_query* q, const double* query, int64_t d, double tau,
                               int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q);

// one single-query search on a workspace of the pool
static as_status search_pooled(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, int64_t* out_idx,
                               double* out_score, int64_t* out_len, double* out_lambda_q) {
    AS_HIP(hipSetDevice(sp->device));
    // (what gang_launch goes by: callers inside as_search on this space right now, and whether two or more were seen lately)
    const int act = sp->active_callers.fetch_add(1, std::memory_order_relaxed) + 1;
    // (gang_width: the most callers seen at once over the last 64 searches or so -- restarted from the current count every 64th)
    if ((sp->gang_tick.fetch_add(1, std::memory_order_relaxed) & 63) == 0 || act > sp->gang_width.load(std::memory_order_relaxed))
        sp->gang_width.store(act, std::memory_order_relaxed);
    if (act >= 2) sp->gang_hint.store(64, std::memory_order_relaxed);
    else if (sp->gang_hint.load(std::memory_order_relaxed) > 0) sp->gang_hint.fetch_sub(1, std::memory_order_relaxed);
    int slot = -1;
    as_query* q = nullptr;
    as_status s = pool_acquire(sp, gr, &slot, &q);
    if (s == AS_OK) {
        s = search_single(sp, gr, q, query, d, tau, out_idx, out_score, out_len, out_lambda_q);
        pool_release(sp, slot);
    }
    sp->active_callers.fetch_sub(1, std::memory_order_relaxed);
    return s;
}

// the graph handle belongs to this space: item graphs have one node per item, feature graphs one per column
static as_status graph_matches(const as_space* sp, const as_graph* gr, const char* who) {
    // a shard of a row-sharded index searches against the graph of all items
    const bool ok = gr->lambda_mode == AS_LAMBDA_FEATURE ? (gr->n == sp->d && gr->nitems >= sp->row_offset + sp->n)
                    : gr->ncols                          ? (gr->row0 == sp->row_offset && gr->n == sp->n && gr->ncols >= gr->row0 + gr->n)
                                                         : gr->n >= sp->row_offset + sp->n;
    if (!ok) {
        set_err("%s: the graph (%lld nodes) was not built for this space (%lld items x %lld features)", who, (long long)gr->n,
                (long long)sp->n, (long long)sp->d);
        return AS_EINVAL;
    }
    return AS_OK;
}

// what the getters of a family's counters share (`counts`: of the space, when there is one)
static as_status counters_out(const char* who, const as_space* sp, int64_t* out, int32_t n, const std::atomic<int64_t>* counts, int len) {
    if (!sp || !out) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    for (int i = 0; i < n && i < len; ++i) out[i] = counts[i].load(std::memory_order_relaxed);
    return AS_OK;
}

int32_t as_space_knn_pipe(const as_space* sp) { return sp ? sp->k2_last_pipe : -1; }
int32_t as_last_scan_int8(const as_space* sp) { return sp && sp->qcache ? as_query_scan_int8(sp->qcache) : 0; }
int64_t as_batch_dual_scans(const as_space* sp) { return sp ? (int64_t)sp->batch_dual_scans.load(std::memory_order_relaxed) : 0; }
int32_t as_last_scan_bits(const as_space* sp) { return sp && sp->qcache ? as_query_scan_bits(sp->qcache) : 8; }

// Debugging aids of the nibble tiles (tests): the image as it lies in HBM, and the dots the last single-query scan kept.
as_status as_debug_nibble_image(const as_space* sp, void* tiles, int64_t tiles_bytes, float* fa4, int64_t nrows, double* info) {
    if (!sp || !info) {
        set_err("as_debug_nibble_image: null argument");
        return AS_EINVAL;
    }
    AS_HIP(hipSetDevice(sp->device));
    bool have = false;
    AS_TRY(space_nib_image(sp, &have));
    info[0] = have ? 1.0 : 0.0;
    info[1] = have ? sp->r4max : 0.0;
    info[2] = (double)(sp->dp8 / 32);
    info[3] = (double)(sp->np + ROW_TILE);
    if (!have) return AS_OK;
    const int64_t all = (sp->np + ROW_TILE) * (sp->dp8 / 2);
    if (tiles) {
        if (tiles_bytes != all) {
            set_err("as_debug_nibble_image: the tiles are %lld bytes", (long long)all);
            return AS_EINVAL;
        }
        AS_HIP(hipMemcpy(tiles, sp->x4, (size_t)all, hipMemcpyDeviceToHost));
    }
    if (fa4) {
        if (nrows < 0 || nrows > sp->np + ROW_TILE) {
            set_err("as_debug_nibble_image: at most %lld rows", (long long)(sp->np + ROW_TILE));
            return AS_EINVAL;
        }
        AS_HIP(hipMemcpy(fa4, sp->fa4, sizeof(float) * (size_t)nrows, hipMemcpyDeviceToHost));
    }
    return AS_OK;
}

// The same for the int8 two-digit image under them: the image and its scales as they lie in HBM, the high-digit tiles, and the two
// maxima the quantiser measured (what every int8 pass prices its dots with).
as_status as_debug_i8_image(const as_space* sp, void* x8, int64_t x8_bytes, float* fa8, int64_t nrows, void* x8h, int64_t x8h_bytes, double* info) {
    if (!sp || !info) {
        set_err("as_debug_i8_image: null argument");
        return AS_EINVAL;
    }
    AS_HIP(hipSetDevice(sp->device));
    bool have = false;
    AS_TRY(space_i8_image(sp, &have));
    const int64_t rows = sp->np + ROW_TILE;
    info[0] = have ? 1.0 : 0.0;
    info[1] = sp->x8 ? sp->u8max : 0.0;
    info[2] = sp->x8 ? sp->v8max : 0.0;
    info[3] = sp->x8 ? sp->coef8 : 0.0;
    info[4] = sp->x8 ? (double)sp->dp8 : 0.0;
    info[5] = (double)rows;
    info[6] = (double)sp->x8_bad;
    if (!have) return AS_OK;
    if (x8) {
        if (x8_bytes != rows * sp->dp8 * 2) {
            set_err("as_debug_i8_image: the image is %lld bytes", (long long)(rows * sp->dp8 * 2));
            return AS_EINVAL;
        }
        AS_HIP(hipMemcpy(x8, sp->x8, (size_t)x8_bytes, hipMemcpyDeviceToHost));
    }
    if (fa8) {
        if (nrows < 0 || nrows > rows) {
            set_err("as_debug_i8_image: at most %lld rows", (long long)rows);
            return AS_EINVAL;
        }
        AS_HIP(hipMemcpy(fa8, sp->fa8, sizeof(float) * (size_t)nrows, hipMemcpyDeviceToHost));
    }
    if (x8h) {
        if (x8h_bytes != rows * sp->dp8) {
            set_err("as_debug_i8_image: the high-digit tiles are %lld bytes", (long long)(rows * sp->dp8));
            return AS_EINVAL;
        }
        bool have_h = false;
        AS_TRY(space_i8h_image(sp, &have_h));
        if (!have_h) {
            set_err("as_debug_i8_image: no memory for the high-digit tiles");
            return AS_ENOMEM;
        }
        AS_HIP(hipMemcpy(x8h, sp->x8h, (size_t)x8h_bytes, hipMemcpyDeviceToHost));
    }
    return AS_OK;
}

int32_t as_last_batch_int8(const as_space* sp) { return sp && sp->qcache_b ? as_query_scan_int8(sp->qcache_b) : 0; }

as_status as_gang_counters(const as_space* sp, int64_t* out, int32_t n) {
    if (!sp || !out) {
        set_err("as_gang_counters: null argument");
        return AS_EINVAL;
    }
    std::lock_guard<std::mutex> lk(sp->gmu);
    for (int i = 0; i < n && i < 4; ++i) out[i] = sp->gang_scans[i + 1];
    for (int i = 4; i < n && i < 10; ++i) out[i] = sp->gang_skip[i - 4].load(std::memory_order_relaxed);
    return AS_OK;
}

int32_t as_search_pool_size(const as_space* sp) {
    if (!sp) return 0;
    std::lock_guard<std::mutex> lk(sp->qmu);
    int n = 0;
    for (int i = 0; i < as_space::QPOOL; ++i) n += sp->qpool[i] ? 1 : 0;
    return n;
}

as_status as_search(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, int64_t* out_idx,
                    double* out_score, int64_t* out_len, double* out_lambda_q) {
    if (!sp || !gr || !query || !out_idx || !out_score) {
        set_err("as_search: null argument");
        return AS_EINVAL;
    }
    if (d != sp->d) {  // src/lib.rs:140-146
        set_err("query length %lld must match nfeatures %lld", (long long)d, (long long)sp->d);
        return AS_EINVAL;
    }
    AS_TRY(graph_matches(sp, gr, "as_search"));
    return search_pooled(sp, gr, query, d, tau, out_idx, out_score, out_len, out_lambda_q);
}

static as_status search_single(const as_space* sp, const as_graph* gr, as_query* q, const double* query, int64_t d, double tau,
                               int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q) {
    (void)gr;
    // mode bit0: fp64 end to end, bit1: wavefront-list selection (candidate buffer overflowed)
    int mode = sp->opts.search_mode & 3;  // tests start directly on a fallback path
    as_status s = AS_OK;
    int64_t cnt[6] = {1, 0, 0, 0, 0, 0};
    for (int attempt = 0; attempt < 3; ++attempt) {
        s = search_once(q, query, d, tau, mode, out_idx, out_score, out_len, out_lambda_q);
        if (s != AS_OK && s != AS_EZEROLAMBDA) break;
        // lambda_q == 0 (no item within eps, proven: the k-NN check below still escalates an unproven empty list) is the
        // reference's panic (src/lib.rs:156-159): no result will be returned, so the scorer's flags of such a query --
        // every item ties at tau = 0 -- must not buy it two more passes over the items
        if (s == AS_EZEROLAMBDA) {
            int ki0 = 0, si0 = 0;
            query_flags(q, &ki0, &si0);
            if (!(ki0 & 1) && !(query_overflow_bits(q) & 1)) break;
        }
        int ki = 0, si = 0;
        query_flags(q, &ki, &si);
        int next = mode;
        if (ki & 2) next |= 2;
        if (((ki & 1) || si) && !sp->opts.force_exact) next |= 1;
        if (next == mode) break;
        dbg("search: fast path not provably exact (knn=%d score=%d), rerunning with mode %d", ki, si, next);
        cnt[2] += (ki & 1) ? 1 : 0;
        cnt[3] += (ki & 2) ? 1 : 0;
        cnt[4] += si ? 1 : 0;
        cnt[5] = 1;
        mode = next;
    }
    cnt[1] = s == AS_EZEROLAMBDA ? 1 : 0;
    {
        std::lock_guard<std::mutex> lk(sp->qmu);
        for (int i = 0; i < 6; ++i) sp->scount[i] += cnt[i];
    }
    if (s == AS_OK && out_lambda_q) dbg("search: qlen=%lld, lambda_q=%.6f", (long long)d, *out_lambda_q);  // src/lib.rs:161-165
    {   // the strongest path has run and the answer still fails its a-posteriori check (more near-ties than fp64
        // can order): it is returned, but never silently -- counted, and reported on stderr once per space
        int ki = 0, si = 0;
        query_flags(q, &ki, &si);
        if (s == AS_OK && ((ki & 1) || (si & 1))) {
            std::lock_guard<std::mutex> lk(sp->qmu);
            if (sp->unproven_searches++ == 0)
                fprintf(stderr, "[pyarrowspace] warning: a search result could not be proven exact (ties at the k-th distance or score "
                                "inside fp64 rounding); see as_unproven_searches()\n");
        }
    }
    return s;
}

// Extension: one query under ntau taus (the evaluation scripts' tau sweeps) -- list j is what as_search returns for taus[j].
// Equal taus are computed once; taus outside [0, 1] (NaN included) and a sweep of one distinct tau take the single search; the
// others share passes of up to TAU_GROUP taus each (search_sweep), and whatever a pass does not serve is redone by the single
// search, with its own escalation.  One workspace of the pool for the whole call; never part of a gang scan.
as_status as_search_taus(const as_space* sp, const as_graph* gr, const double* query, int64_t d, const double* taus, int64_t ntau,
                         int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q) {
    if (!sp || !gr || !query || ntau < 0 || (ntau > 0 && (!taus || !out_idx || !out_score || !out_len))) {
        set_err("as_search_taus: null argument");
        return AS_EINVAL;
    }
    if (d != sp->d) {
        set_err("query length %lld must match nfeatures %lld", (long long)d, (long long)sp->d);
        return AS_EINVAL;
    }
    AS_TRY(graph_matches(sp, gr, "as_search_taus"));
    if (ntau == 0) return AS_OK;
    sp->sweep_count[0].fetch_add(1, std::memory_order_relaxed);
    const int64_t topk = std::min<int64_t>(gr->gp.topk, sp->n);
    const int64_t ls = std::max<int64_t>(topk, 1);
    // distinct taus (bit patterns), in order of first appearance; the shared passes take those in [0, 1]
    std::vector<double> uniq;
    std::vector<int64_t> slot((size_t)ntau);
    for (int64_t j = 0; j < ntau; ++j) {
        int64_t u = 0;
        while (u < (int64_t)uniq.size() && memcmp(&uniq[u], &taus[j], sizeof(double)) != 0) ++u;
        if (u == (int64_t)uniq.size()) uniq.push_back(taus[j]);
        slot[j] = u;
    }
    const int64_t nu = (int64_t)uniq.size();
    std::vector<int64_t> uidx((size_t)(nu * ls)), ulen((size_t)nu, 0);
    std::vector<double> usc((size_t)(nu * ls));
    std::vector<int> done((size_t)nu, 0);
    std::vector<int64_t> shared;
    for (int64_t u = 0; u < nu; ++u)
        if (uniq[u] >= 0.0 && uniq[u] <= 1.0) shared.push_back(u);
    if (shared.size() < 2) shared.clear();   // (one distinct tau: the single search is the whole sweep)
    AS_HIP(hipSetDevice(sp->device));
    int ps = -1;
    as_query* q = nullptr;
    AS_TRY(pool_acquire(sp, gr, &ps, &q));
    as_status s = AS_OK;
    double lq = 0.0;
    int64_t passes = 0, redone = 0;
    for (size_t g0 = 0; g0 < shared.size() && s == AS_OK; g0 += TAU_GROUP) {
        const int nt = (int)std::min<size_t>(TAU_GROUP, shared.size() - g0);
        if (nt < 2) break;   // (a last group of one: the single search below)
        double gt[TAU_GROUP];
        int served[TAU_GROUP];
        int64_t glen[TAU_GROUP];
        for (int j = 0; j < nt; ++j) gt[j] = uniq[shared[g0 + j]];
        std::vector<int64_t> sidx((size_t)(nt * ls));
        std::vector<double> ssc((size_t)(nt * ls));
        s = search_sweep(q, query, d, gt, nt, ls, sidx.data(), ssc.data(), glen, &lq, served);
        int nserved = 0;
        for (int j = 0; j < nt; ++j) {
            if (!served[j]) continue;
            nserved += 1;
            const int64_t u = shared[g0 + j];
            done[u] = 1;
            ulen[u] = glen[j];
            for (int64_t t = 0; t < glen[j]; ++t) {
                uidx[u * ls + t] = sidx[j * ls + t];
                usc[u * ls + t] = ssc[j * ls + t];
            }
        }
        if (nserved > 0) passes += 1;
        if (s == AS_OK) redone += nt - nserved;
    }
    for (int64_t u = 0; u < nu && s == AS_OK; ++u) {
        if (done[u]) continue;
        s = search_single(sp, gr, q, query, d, uniq[u], &uidx[u * ls], &usc[u * ls], &ulen[u], &lq);
        done[u] = 1;
    }
    pool_release(sp, ps);
    sp->sweep_count[1].fetch_add(passes, std::memory_order_relaxed);
    sp->sweep_count[2].fetch_add(redone, std::memory_order_relaxed);
    if (out_lambda_q) *out_lambda_q = lq;
    if (s != AS_OK) return s;   // (AS_EZEROLAMBDA: lambda_q does not depend on tau -- every tau would panic)
    for (int64_t j = 0; j < ntau; ++j) {
        const int64_t u = slot[j];
        for (int64_t t = 0; t < ulen[u]; ++t) {
            out_idx[j * topk + t] = uidx[u * ls + t];
            out_score[j * topk + t] = usc[u * ls + t];
        }
        out_len[j] = ulen[u];
    }
    return AS_OK;
}

as_status as_sweep_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_sweep_counters", sp, out, n, sp ? sp->sweep_count : nullptr, 3);
}

// ---------------------------------------------------------------- the filtered call frame (extensions)
// What every filtered entry point is made of (subset / items, lists, range, fused, grouped and diversified search, their batched
// and tau-sweep forms), in the order each of them keeps: its own null-argument test and the zeroing of out_len / out_ngroups; the
// refusals before anything is launched (own_subset, ids_in_range, subset_checks -- which of the first two comes before the third
// is the entry point's own, and stays); its `calls` counter; ONE lambda_q step (lambda_step, batch_lambda_step); the work buffers
// (Candidates); the run; the copies of repeated taus (copy_repeated_lists, copy_repeated_rows).

// what every filtered form checks alike (the tau sweeps: every tau of the list)
static as_status subset_checks(const char* who, const as_space* sp, const as_graph* gr, int64_t d, const double* taus, int64_t ntau) {
    if (d != sp->d) {
        set_err("query length %lld must match nfeatures %lld", (long long)d, (long long)sp->d);
        return AS_EINVAL;
    }
    for (int64_t j = 0; j < ntau; ++j)
        if (!std::isfinite(taus[j])) {
            set_err("%s: tau must be finite", who);
            return AS_EINVAL;
        }
    AS_TRY(graph_matches(sp, gr, who));
    if (sp->row_offset != 0 || gr->ncols) {
        set_err("%s: a shard of a row-sharded index is not supported", who);
        return AS_EUNSUPPORTED;
    }
    return AS_OK;
}
// the first of m ids outside [0, n), or null
static const int64_t* bad_id(const as_space* sp, const int64_t* ids, int64_t m) {
    for (int64_t i = 0; i < m; ++i)
        if (ids[i] < 0 || ids[i] >= sp->n) return ids + i;
    return nullptr;
}
static as_status ids_in_range(const char* who, const as_space* sp, const int64_t* ids, int64_t m) {
    if (const int64_t* bad = bad_id(sp, ids, m)) {
        set_err("%s: id %lld is outside [0, %lld)", who, (long long)*bad, (long long)sp->n);
        return AS_EINVAL;
    }
    return AS_OK;
}
// ids that passed ids_in_range, narrowed (item ids fit 32 bits: space_new refuses n >= 2^31)
static as_status checked_ids(const char* who, const int64_t* ids_host, int64_t m, std::vector<int32_t>& ids) {
    if (m >= (int64_t)1 << 31) {
        set_err("%s: %lld ids exceed the supported maximum of 2^31 - 1 per call", who, (long long)m);
        return AS_EUNSUPPORTED;
    }
    try {
        ids.assign(ids_host, ids_host + m);
    } catch (const std::bad_alloc&) {
        set_err("%s: out of host memory for %lld ids", who, (long long)m);
        return AS_ENOMEM;
    }
    return AS_OK;
}
// a subset handle (null: none was given) belongs to the space of the call
static as_status own_subset(const char* who, const as_space* sp, const as_subset* sub) {
    if (sub && sub->sp != sp) {
        set_err("%s: the subset was made for another space", who);
        return AS_EINVAL;
    }
    return AS_OK;
}
// entries of a hit list over m candidates
static int64_t hits_bound(const as_space* sp, const as_graph* gr, int64_t m) {
    return std::min<int64_t>(std::min<int64_t>(gr->gp.topk, sp->n), m);
}

// lambda_q of one query: ONE single search on a workspace of the pool, hits discarded -- its escalation, its AS_EZEROLAMBDA, its
// lambda_q, published whatever the status.  `steps`: the family's counter of lambda_q steps, where it has one.
static as_status lambda_step(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, std::atomic<int64_t>* steps,
                             double* lq, double* out_lambda_q) {
    if (steps) steps->fetch_add(1, std::memory_order_relaxed);
    int64_t hidx[SUBSET_TOPK], hlen = 0;
    double hsc[SUBSET_TOPK];
    const as_status s = search_pooled(sp, gr, query, d, tau, hidx, hsc, &hlen, lq);
    if (out_lambda_q) *out_lambda_q = *lq;
    return s;
}
// lambda_q and the status of every query of a batched form: ONE as_search_batch call over all b queries, hits discarded -- its
// escalation, its values, published once it has returned AS_OK.  (It has then released sp->bmu: see Candidates.)
static as_status batch_lambda_step(const char* who, const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d,
                                   double tau, std::atomic<int64_t>* steps, std::vector<double>& lq, std::vector<int32_t>& st,
                                   double* out_lambda_q, int32_t* out_status) {
    if (b == 0) return AS_OK;
    if (steps) steps->fetch_add(1, std::memory_order_relaxed);
    const int64_t topk = std::max<int64_t>(hits_bound(sp, gr, sp->n), 1);
    std::vector<int64_t> hidx, hlen;
    std::vector<double> hsc;
    try {
        hidx.resize((size_t)(b * topk));
        hsc.resize((size_t)(b * topk));
        hlen.resize((size_t)b);
        lq.assign((size_t)b, 0.0);
        st.assign((size_t)b, 0);
    } catch (const std::bad_alloc&) {
        set_err("%s: out of host memory for %lld queries", who, (long long)b);
        return AS_ENOMEM;
    }
    AS_TRY(as_search_batch(sp, gr, queries, b, d, tau, hidx.data(), hsc.data(), hlen.data(), lq.data(), st.data()));
    for (int64_t i = 0; i < b; ++i) {
        if (out_lambda_q) out_lambda_q[i] = lq[i];
        if (out_status) out_status[i] = st[i];
    }
    return AS_OK;
}

// the space's work buffers for m ids (under sp->smu): grown on demand, never per call otherwise; the ids uploaded
static as_status score_ws_ids(const as_space* sp, const int32_t* ids, int64_t m) {
    if (!sp->score_ws || sp->score_ws->cap < m) {
        subset_work_free(sp->score_ws);
        sp->score_ws = nullptr;
        int64_t cap = 1024;
        while (cap < m) cap *= 2;
        AS_TRY(subset_work_create(sp, cap, &sp->score_ws));
    }
    return subset_set_ids(sp->score_ws, ids, m);
}
// the space's own subset of all items (made on first use under sp->rmu, kept; no host id list: position == id)
static as_status all_items(const as_space* sp, const as_subset** out) {
    std::lock_guard<std::mutex> lk(sp->rmu);
    if (!sp->range_all) {
        AS_HIP(hipSetDevice(sp->device));
        std::vector<int32_t> ids;
        as_subset* all = nullptr;
        try {
            ids.resize((size_t)sp->n);
            all = new as_subset();
        } catch (const std::bad_alloc&) {
            set_err("range: out of host memory for %lld ids", (long long)sp->n);
            return AS_ENOMEM;
        }
        for (int64_t i = 0; i < sp->n; ++i) ids[(size_t)i] = (int32_t)i;
        all->sp = sp;
        all->m = sp->n;
        as_status s = subset_work_create(sp, all->m, &all->w);
        if (s == AS_OK) s = subset_set_ids(all->w, ids.data(), all->m);
        if (s != AS_OK) {
            as_subset_free(all);
            return s;
        }
        sp->range_all = all;
    }
    *out = sp->range_all;
    return AS_OK;
}

namespace {
// The candidates of one filtered call and the work buffers they are scored on, held for the call.  Three sources: the caller's
// subset handle (under the handle's mutex); neither a handle nor ids: the space's subset of all items (under that handle's
// mutex); the caller's ids, checked and narrowed: sp->score_ws with the ids uploaded (under sp->smu).  The space's device is made
// current under the lock.  `status` is looked at before anything is run; the run's status goes through fail(), so that a failed
// run leaves nothing on the work's stream when the lock is released.
// The lock rules of the filtered forms: the lambda_q step comes first and has returned -- as_search_batch has released sp->bmu --
// before a handle's mutex, sp->smu or sp->lmu (the lists' buffers) is taken; sp->rmu guards only the creation of the subset of
// all items and is released before that handle's mutex is taken; no two of these mutexes are ever held together.  One mutex is
// taken inside a handle's: sp->fmu, by the diffusion forms (their recurrence runs on the space's diffusion buffers, their selection
// on the handle's), always in that order; nothing takes a handle's mutex, sp->smu or sp->lmu under sp->fmu.
struct Candidates {
    const as_space* sp;
    SubsetWork* w = nullptr;
    int64_t m = 0;
    const int64_t* ids = nullptr;   // the handle's host ids (null: position == id, or the caller's own list)
    as_status status = AS_OK;
    std::unique_lock<std::mutex> lk;
    // the caller's subset handle, or (null) the space's subset of all items
    Candidates(const char* who, const as_space* sp_, const as_subset* sub) : sp(sp_) {
        if (!sub && (status = all_items(sp, &sub)) != AS_OK) return;
        if (!hold(who, sub->mu)) return;
        w = sub->w;
        m = sub->m;
        ids = sub->ids;
    }
    // the caller's m32 ids, narrowed, in sp->score_ws
    Candidates(const char* who, const as_space* sp_, const int32_t* ids32, int64_t m32) : sp(sp_) {
        if (!hold(who, sp->smu)) return;
        status = score_ws_ids(sp, ids32, m32);
        w = sp->score_ws;
        m = m32;
    }
    as_status fail(as_status s) const {
        if (s != AS_OK && w) (void)hipStreamSynchronize(w->stream);
        return s;
    }

  private:
    bool hold(const char* who, std::mutex& mu) {
        lk = std::unique_lock<std::mutex>(mu);
        if (hipSetDevice(sp->device) == hipSuccess) return true;
        set_err("%s: hipSetDevice failed", who);
        status = AS_EHIP;
        return false;
    }
};

// The distinct taus of a sweep (bit patterns) in order of first appearance: row[u] = the entry of the list uniq[u] was taken
// from, first[j] = the first entry with taus[j]'s bits.  Equal taus are computed once and copied (below).
struct TauSet {
    std::vector<double> uniq;
    std::vector<int64_t> row, first;
    TauSet(const double* taus, int64_t ntau) : first((size_t)ntau) {
        for (int64_t j = 0; j < ntau; ++j) {
            size_t u = 0;
            while (u < uniq.size() && memcmp(&uniq[u], &taus[j], sizeof(double)) != 0) ++u;
            if (u == uniq.size()) {
                uniq.push_back(taus[j]);
                row.push_back(j);
            }
            first[(size_t)j] = row[u];
        }
    }
    int64_t ntau() const { return (int64_t)first.size(); }
    int64_t size() const { return (int64_t)uniq.size(); }
};
}  // namespace

// Equal taus are copies of the first one's list (b queries x ntau lists at stride kk) ...
static void copy_repeated_lists(const TauSet& ts, int64_t b, int64_t kk, const int32_t* skip, int64_t* out_idx, double* out_score,
                                int64_t* out_len) {
    for (int64_t i = 0; i < b; ++i) {
        if (skip && skip[i] == AS_EZEROLAMBDA) continue;
        for (int64_t j = 0; j < ts.ntau(); ++j) {
            const int64_t f = i * ts.ntau() + ts.first[(size_t)j], p = i * ts.ntau() + j;
            if (f == p) continue;
            for (int64_t t = 0; t < out_len[f]; ++t) {
                out_idx[p * kk + t] = out_idx[f * kk + t];
                out_score[p * kk + t] = out_score[f * kk + t];
            }
            out_len[p] = out_len[f];
        }
    }
}
// ... or of its score row: query i's ntau rows of m entries (offs: of offs[i + 1] - offs[i] entries, behind the rows of the
// queries before it).  `skip`: the status of every query, where one with AS_EZEROLAMBDA is left out -- nothing of it was
// written, its rows stay unwritten.
static void copy_repeated_rows(const TauSet& ts, int64_t b, int64_t m, const int64_t* offs, const int32_t* skip, double* out) {
    for (int64_t i = 0; i < b; ++i) {
        if (skip && skip[i] == AS_EZEROLAMBDA) continue;
        const int64_t mi = offs ? offs[i + 1] - offs[i] : m;
        double* blk = out + ts.ntau() * (offs ? offs[i] : i * m);
        for (int64_t j = 0; j < ts.ntau() && mi > 0; ++j)
            if (ts.first[(size_t)j] != j) memcpy(blk + j * mi, blk + ts.first[(size_t)j] * mi, sizeof(double) * (size_t)mi);
    }
}

// ---------------------------------------------------------------- filtered search (extension; kernels: as_subset.hip)

as_status as_subset_create(const as_space* sp, const int64_t* ids_host, int64_t m, as_subset** out) {
    if (!sp || !out || m < 0 || (m > 0 && !ids_host)) {
        set_err("as_subset_create: null argument");
        return AS_EINVAL;
    }
    *out = nullptr;
    AS_TRY(ids_in_range("as_subset_create", sp, ids_host, m));
    std::vector<int32_t> ids;   // (item ids fit 32 bits: space_new refuses n >= 2^31)
    as_subset* sub = nullptr;
    try {
        ids.assign(ids_host, ids_host + m);
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        sub = new as_subset();
        sub->ids = new int64_t[ids.size() + 1];
    } catch (const std::bad_alloc&) {
        delete sub;
        set_err("as_subset_create: out of host memory for %lld ids", (long long)m);
        return AS_ENOMEM;
    }
    sub->sp = sp;
    sub->m = (int64_t)ids.size();
    for (int64_t i = 0; i < sub->m; ++i) sub->ids[i] = ids[i];
    as_status s = hipSetDevice(sp->device) == hipSuccess ? AS_OK : AS_EHIP;
    if (s != AS_OK) set_err("as_subset_create: hipSetDevice failed");
    if (s == AS_OK) s = subset_work_create(sp, sub->m, &sub->w);
    if (s == AS_OK) s = subset_set_ids(sub->w, ids.data(), sub->m);
    if (s != AS_OK) {
        as_subset_free(sub);
        return s;
    }
    *out = sub;
    return AS_OK;
}

int64_t as_subset_size(const as_subset* sub) { return sub ? sub->m : 0; }

as_status as_subset_ids(const as_subset* sub, int64_t* out) {
    if (!sub || (sub->m > 0 && !out)) {
        set_err("as_subset_ids: null argument");
        return AS_EINVAL;
    }
    for (int64_t i = 0; i < sub->m; ++i) out[i] = sub->ids[i];
    return AS_OK;
}

void as_subset_free(as_subset* sub) {
    if (!sub) return;
    subset_work_free(sub->w);
    delete[] sub->ids;
    delete sub;
}

void as_subset_set_timing(as_subset* sub, int32_t enabled) {
    if (!sub || !sub->w) return;
    std::lock_guard<std::mutex> lk(sub->mu);
    sub->w->timing = enabled ? 1 : 0;
}
double as_subset_kernel_us(const as_subset* sub) {
    if (!sub || !sub->w) return 0.0;
    std::lock_guard<std::mutex> lk(sub->mu);
    return sub->w->kernel_us;
}

as_status as_search_subset(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, const as_subset* sub,
                           int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q) {
    if (!sp || !gr || !query || !sub || !out_len || (sub->m > 0 && (!out_idx || !out_score))) {
        set_err("as_search_subset: null argument");
        return AS_EINVAL;
    }
    *out_len = 0;
    AS_TRY(own_subset("as_search_subset", sp, sub));
    double lq = 0.0;
    if (out_lambda_q) *out_lambda_q = lq;   // (the two plain single forms publish lambda_q = 0 with a refusal of the checks below)
    AS_TRY(subset_checks("as_search_subset", sp, gr, d, &tau, 1));
    AS_TRY(lambda_step(sp, gr, query, d, tau, nullptr, &lq, out_lambda_q));
    if (sub->m == 0) return AS_OK;
    Candidates c("as_search_subset", sp, sub);
    AS_TRY(c.status);
    as_status s = subset_score(sp, c.w, c.m, query, tau, lq);
    if (s == AS_OK) s = subset_select(c.w, c.m, hits_bound(sp, gr, c.m), out_idx, out_score, out_len);
    return c.fail(s);
}

as_status as_score_items(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, const int64_t* ids_host,
                         int64_t m, double* out_scores, double* out_lambda_q) {
    if (!sp || !gr || !query || m < 0 || (m > 0 && (!ids_host || !out_scores))) {
        set_err("as_score_items: null argument");
        return AS_EINVAL;
    }
    AS_TRY(ids_in_range("as_score_items", sp, ids_host, m));
    double lq = 0.0;
    if (out_lambda_q) *out_lambda_q = lq;   // (as in as_search_subset)
    AS_TRY(subset_checks("as_score_items", sp, gr, d, &tau, 1));
    AS_TRY(lambda_step(sp, gr, query, d, tau, nullptr, &lq, out_lambda_q));
    if (m == 0) return AS_OK;
    std::vector<int32_t> ids;
    AS_TRY(checked_ids("as_score_items", ids_host, m, ids));
    Candidates c("as_score_items", sp, ids.data(), m);
    AS_TRY(c.status);
    as_status s = subset_score(sp, c.w, m, query, tau, lq);
    if (s == AS_OK) s = subset_scores_out(c.w, m, out_scores);
    return c.fail(s);
}

// the batched workspaces for b > 1 queries (under sp->bmu); *unit = the passes launched together (2: a pair sharing one scan)
static as_status batch_workspaces(const as_space* sp, const as_graph* gr, int64_t b, int* unit) {
    if (sp->qcache_b && sp->qcache_b_gr != gr) {
        for (as_query** w : {&sp->qcache_b, &sp->qcache_b2, &sp->qcache_b3, &sp->qcache_b4}) {
            if (*w) as_query_free(*w);
            *w = nullptr;
        }
    }
    if (!sp->qcache_b) {
        AS_TRY(query_create(sp, gr, QUERY_BATCH, &sp->qcache_b));
        sp->qcache_b_gr = gr;
    }
    // More than one pass: a second workspace.  Rows of up to 768 columns: the two launch their passes as a PAIR, one scan for
    // both (64 queries per read of the items: search_batch_launch_pair); more than one pair: a second pair of workspaces, pair
    // p + 1 is queued before pair p is waited for.  Wider rows (a scan serves one workspace): the passes alternate between
    // the two workspaces -- pass p + 1 is queued before pass p is waited for.  (No memory: fewer workspaces, the same results.)
    static const bool no_pipe = getenv("ARROWSPACE_NO_BATCH_PIPELINE") != nullptr;
    static const bool no_dual = getenv("ARROWSPACE_NO_BATCH_DUAL") != nullptr;
    const bool pairs = !no_dual && (sp->dp + 63) / 64 * 64 / 2 <= 4 * 3 * 32 && gr->lambda_mode != AS_LAMBDA_FEATURE;
    if (b > QUERY_BATCH && !sp->qcache_b2 && !no_pipe) {
        if (query_create(sp, gr, QUERY_BATCH, &sp->qcache_b2) != AS_OK) sp->qcache_b2 = nullptr;
    }
    if (pairs && b > 2 * QUERY_BATCH && sp->qcache_b2 && !sp->qcache_b4 && !no_pipe) {
        if (!sp->qcache_b3 && query_create(sp, gr, QUERY_BATCH, &sp->qcache_b3) != AS_OK) sp->qcache_b3 = nullptr;
        if (sp->qcache_b3 && query_create(sp, gr, QUERY_BATCH, &sp->qcache_b4) != AS_OK) sp->qcache_b4 = nullptr;
    }
    *unit = pairs && sp->qcache_b2 && b > QUERY_BATCH ? 2 : 1;
    return AS_OK;
}

as_status as_search_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                          int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || !queries || !out_idx || !out_score || !out_len) {
        set_err("as_search_batch: null argument");
        return AS_EINVAL;
    }
    if (d != sp->d) {
        set_err("query length %lld must match nfeatures %lld", (long long)d, (long long)sp->d);
        return AS_EINVAL;
    }
    AS_TRY(graph_matches(sp, gr, "as_search_batch"));
    const int64_t topk = std::min<int64_t>(gr->gp.topk, sp->n);
    std::lock_guard<std::mutex> lock(sp->bmu);   // (the batched workspaces; single-query fallbacks below go through the pool)
    AS_HIP(hipSetDevice(sp->device));
    int32_t st_chunk[QUERY_BATCH];
    // the slots of a pass the batched fast path did not prove exact (or all of them: batching unavailable) on the single-query path
    auto singles = [&](int64_t i0, int nb) -> as_status {
        for (int t = 0; t < nb; ++t) {
            const int64_t i = i0 + t;
            if (st_chunk[t] == -1) {
                double lq = 0.0;
                const as_status s1 = search_pooled(sp, gr, queries + i * d, d, tau, out_idx + i * topk, out_score + i * topk, out_len + i, &lq);
                if (out_lambda_q) out_lambda_q[i] = lq;
                st_chunk[t] = (int32_t)s1;
                if (s1 != AS_OK && s1 != AS_EZEROLAMBDA) return s1;
            }
            if (st_chunk[t] == AS_EZEROLAMBDA) out_len[i] = 0;
            if (out_status) out_status[i] = st_chunk[t];
        }
        return AS_OK;
    };
    // the batched pass serves QUERY_BATCH queries per read of the items (MFMA pass; rows wider than 768 floats in
    // K-chunk passes of the same kernel): fp32 fast path only
    if (sp->opts.force_exact || (sp->opts.search_mode & 3) != 0 || b <= 1) {
        for (int64_t i0 = 0; i0 < b; i0 += QUERY_BATCH) {
            for (int t = 0; t < QUERY_BATCH; ++t) st_chunk[t] = -1;
            AS_TRY(singles(i0, (int)std::min<int64_t>(QUERY_BATCH, b - i0)));
        }
        return AS_OK;
    }
    int unit = 1;   // passes launched together
    AS_TRY(batch_workspaces(sp, gr, b, &unit));
    int64_t passes = 0;
    static const bool timing = getenv("ARROWSPACE_DEBUG") != nullptr;   // host time of the two halves of a pass, per call
    double t_launch = 0.0, t_collect = 0.0;
    auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    AS_TRY(batch_passes(
        sp, unit, b,
        [&](as_query* w0, int64_t i0, int nb0, as_query* w1, int64_t i1, int nb1) -> as_status {
            const double t0 = timing ? now() : 0.0;
            const as_status s = w1 ? search_batch_launch_pair(w0, w1, queries + i0 * d, nb0, queries + i1 * d, nb1, d, tau)
                                   : search_batch_launch(w0, queries + i0 * d, nb0, d, tau);
            if (timing) t_launch += now() - t0;
            return s;
        },
        [&](as_query* w, int64_t i0, int nb) -> as_status {
            const double t1 = timing ? now() : 0.0;
            const as_status s = search_batch_collect(w, nb, tau, topk, out_idx + i0 * topk, out_score + i0 * topk, out_len + i0,
                                                     out_lambda_q ? out_lambda_q + i0 : nullptr, st_chunk);
            if (timing) t_collect += now() - t1;
            passes += 1;
            return s != AS_OK ? s : singles(i0, nb);
        }));
    if (timing) dbg("as_search_batch: %lld passes, host time per pass: launch half %.0f us, collect half (with its wait) %.0f us",
                    (long long)passes, t_launch / std::max<int64_t>(passes, 1), t_collect / std::max<int64_t>(passes, 1));
    return AS_OK;
}

// The batched filtered forms: the single forms' checks and messages.

as_status as_search_subset_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                 const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q,
                                 int32_t* out_status) {
    if (!sp || !gr || !sub || b < 0 || (b > 0 && (!queries || !out_len || (sub->m > 0 && (!out_idx || !out_score))))) {
        set_err("as_search_subset_batch: null argument");
        return AS_EINVAL;
    }
    for (int64_t i = 0; i < b; ++i) out_len[i] = 0;
    AS_TRY(own_subset("as_search_subset_batch", sp, sub));
    AS_TRY(subset_checks("as_search_subset_batch", sp, gr, d, &tau, 1));
    std::vector<double> lq;
    std::vector<int32_t> st;
    AS_TRY(batch_lambda_step("as_search_subset_batch", sp, gr, queries, b, d, tau, nullptr, lq, st, out_lambda_q, out_status));
    if (b == 0 || sub->m == 0) return AS_OK;
    const int64_t kk = hits_bound(sp, gr, sub->m);
    Candidates c("as_search_subset_batch", sp, sub);
    AS_TRY(c.status);
    return c.fail(subset_batch_run(sp, c.w, c.m, queries, b, lq.data(), st.data(), tau, kk, kk, out_idx, out_score, out_len, nullptr));
}

as_status as_score_items_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                               const int64_t* ids_host, int64_t m, double* out_scores, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || b < 0 || m < 0 || (b > 0 && !queries) || (m > 0 && !ids_host) || (b > 0 && m > 0 && !out_scores)) {
        set_err("as_score_items_batch: null argument");
        return AS_EINVAL;
    }
    AS_TRY(ids_in_range("as_score_items_batch", sp, ids_host, m));
    AS_TRY(subset_checks("as_score_items_batch", sp, gr, d, &tau, 1));
    std::vector<double> lq;
    std::vector<int32_t> st;
    AS_TRY(batch_lambda_step("as_score_items_batch", sp, gr, queries, b, d, tau, nullptr, lq, st, out_lambda_q, out_status));
    if (b == 0 || m == 0) return AS_OK;
    std::vector<int32_t> ids;
    AS_TRY(checked_ids("as_score_items_batch", ids_host, m, ids));
    Candidates c("as_score_items_batch", sp, ids.data(), m);
    AS_TRY(c.status);
    return c.fail(subset_batch_run(sp, c.w, m, queries, b, lq.data(), st.data(), tau, 0, 0, nullptr, nullptr, nullptr, out_scores));
}

// ---------------------------------------------------------------- range search (extension; as_range.hip)
static as_range* range_new(bool count_only) {
    as_range* r = new (std::nothrow) as_range();
    if (!r) {
        set_err("range: out of host memory");
        return nullptr;
    }
    try {
        r->offs.push_back(0);
    } catch (const std::bad_alloc&) {
        delete r;
        set_err("range: out of host memory");
        return nullptr;
    }
    r->count_only = count_only;
    return r;
}
// `n` empty lists behind those the answer holds
static as_status range_pad(as_range* r, int64_t n) {
    try {
        r->offs.resize(r->offs.size() + (size_t)n, r->offs.back());
    } catch (const std::bad_alloc&) {
        set_err("range: out of host memory for the answer");
        return AS_ENOMEM;
    }
    r->nq += n;
    return AS_OK;
}
static void range_counts_add(const as_space* sp, const int64_t* counts, double us) {
    for (int i = 0; i < 4; ++i) sp->range_count[1 + i].fetch_add(counts[i], std::memory_order_relaxed);
    sp->range_us.store(us, std::memory_order_relaxed);
}

as_status as_search_range(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, double min_score,
                          const as_subset* sub, int32_t count_only, as_range** out, double* out_lambda_q) {
    if (out) *out = nullptr;
    if (!sp || !gr || !query || !out) {
        set_err("as_search_range: null argument");
        return AS_EINVAL;
    }
    if (min_score != min_score) {
        set_err("as_search_range: min_score must not be NaN");
        return AS_EINVAL;
    }
    AS_TRY(own_subset("as_search_range", sp, sub));
    AS_TRY(subset_checks("as_search_range", sp, gr, d, &tau, 1));
    sp->range_count[0].fetch_add(1, std::memory_order_relaxed);
    double lq = 0.0;
    AS_TRY(lambda_step(sp, gr, query, d, tau, &sp->range_count[5], &lq, out_lambda_q));
    as_range* res = range_new(count_only != 0);
    if (!res) return AS_ENOMEM;
    as_status s = AS_OK;
    if (sub && sub->m == 0) s = range_pad(res, 1);
    else {
        Candidates c("as_search_range", sp, sub);
        if ((s = c.status) == AS_OK) {
            int64_t counts[4] = {0, 0, 0, 0};
            double us = 0.0;
            s = subset_score(sp, c.w, c.m, query, tau, lq);
            if (s == AS_OK) s = range_compact(c.w, c.w->scores, c.m, c.m, 1, &min_score, count_only != 0, c.ids, res, counts, &us);
            s = c.fail(s);
            range_counts_add(sp, counts, us);
        }
    }
    if (s != AS_OK) {
        delete res;
        return s;
    }
    *out = res;
    return AS_OK;
}

namespace {
struct RangeSink {
    const Candidates* on;
    const double* thr;   // [b]: NaN for a query without an answer
    bool count_only;
    as_range* res;
    int64_t counts[4];
    double us;
};
as_status range_sink_chunk(void* ctx, SubsetWork* w, int64_t i0, int64_t nb, const double* scores, int64_t ld) {
    RangeSink* k = (RangeSink*)ctx;
    return range_compact(w, scores, ld, k->on->m, nb, k->thr + i0, k->count_only, k->on->ids, k->res, k->counts, &k->us);
}
}  // namespace

as_status as_search_range_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                const double* min_scores, const as_subset* sub, int32_t count_only, as_range** out, double* out_lambda_q,
                                int32_t* out_status) {
    if (out) *out = nullptr;
    if (!sp || !gr || !out || b < 0 || (b > 0 && (!queries || !min_scores))) {
        set_err("as_search_range_batch: null argument");
        return AS_EINVAL;
    }
    for (int64_t i = 0; i < b; ++i)
        if (min_scores[i] != min_scores[i]) {
            set_err("as_search_range_batch: min_scores[%lld] must not be NaN", (long long)i);
            return AS_EINVAL;
        }
    AS_TRY(own_subset("as_search_range_batch", sp, sub));
    AS_TRY(subset_checks("as_search_range_batch", sp, gr, d, &tau, 1));
    sp->range_count[0].fetch_add(1, std::memory_order_relaxed);
    as_range* res = range_new(count_only != 0);
    if (!res) return AS_ENOMEM;
    std::vector<double> lq, thr;
    std::vector<int32_t> st;
    as_status s = batch_lambda_step("as_search_range_batch", sp, gr, queries, b, d, tau, &sp->range_count[5], lq, st, out_lambda_q, out_status);
    if (s == AS_OK) {
        try {
            thr.assign(min_scores, min_scores + b);
        } catch (const std::bad_alloc&) {
            set_err("as_search_range_batch: out of host memory for %lld queries", (long long)b);
            s = AS_ENOMEM;
        }
    }
    if (s == AS_OK && b > 0) {
        if (sub && sub->m == 0) s = range_pad(res, b);
        else {
            // a zero-lambda query's row of a chunk holds no answer: against a NaN threshold nothing in it survives
            for (int64_t i = 0; i < b; ++i)
                if (st[i] == AS_EZEROLAMBDA) thr[i] = std::numeric_limits<double>::quiet_NaN();
            const Candidates c("as_search_range_batch", sp, sub);
            if ((s = c.status) == AS_OK) {
                RangeSink k{&c, thr.data(), count_only != 0, res, {0, 0, 0, 0}, 0.0};
                const SubsetChunkSink sink{range_sink_chunk, &k};
                s = c.fail(subset_batch_run(sp, c.w, c.m, queries, b, lq.data(), st.data(), tau, 0, 0, nullptr, nullptr, nullptr, nullptr, &sink));
                range_counts_add(sp, k.counts, k.us);
            }
        }
    }
    if (s != AS_OK) {
        delete res;
        return s;
    }
    *out = res;
    return AS_OK;
}

int64_t as_range_queries(const as_range* r) { return r ? r->nq : 0; }
int64_t as_range_total(const as_range* r) { return r ? r->offs.back() : 0; }
as_status as_range_offsets(const as_range* r, int64_t* out) {
    if (!r || !out) {
        set_err("as_range_offsets: null argument");
        return AS_EINVAL;
    }
    for (int64_t i = 0; i <= r->nq; ++i) out[i] = r->offs[(size_t)i];
    return AS_OK;
}
as_status as_range_copy(const as_range* r, int64_t* out_idx, double* out_score) {
    if (!r || (r->offs.back() > 0 && (!out_idx || !out_score))) {
        set_err("as_range_copy: null argument");
        return AS_EINVAL;
    }
    if (r->count_only) {
        set_err("as_range_copy: the answer of a count_only call holds no entries");
        return AS_EINVAL;
    }
    for (size_t e = 0; e < r->idx.size(); ++e) {
        out_idx[e] = r->idx[e];
        out_score[e] = r->score[e];
    }
    return AS_OK;
}
void as_range_free(as_range* r) { delete r; }
as_status as_range_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_range_counters", sp, out, n, sp ? sp->range_count : nullptr, 6);
}
double as_range_kernel_us(const as_space* sp) { return sp ? sp->range_us.load(std::memory_order_relaxed) : 0.0; }

// ---------------------------------------------------------------- fused multi-query search (extension; as_fused.hip)
namespace {
// What both forms refuse before anything is launched, then lambda_q and the status of every vector from ONE as_search_batch call
// over the j vectors, then S13's zero-lambda rule.  `wts`: the caller's weights, or 1/j each.  calls, steps: the family's counters
// of calls that passed their checks and of lambda_q steps (steps may be null).
as_status fused_prepare(const char* who, const as_space* sp, const as_graph* gr, const double* queries, int64_t j, int64_t d, double tau,
                        const double* weights, int32_t mode, int32_t skip_zero, const as_subset* sub, double* out_lambda_q, int32_t* out_status,
                        std::vector<double>& wts, std::vector<double>& lq, std::vector<int32_t>& st, std::atomic<int64_t>* calls,
                        std::atomic<int64_t>* steps) {
    if (j <= 0) {
        set_err("%s: j must be >= 1, got %lld", who, (long long)j);
        return AS_EINVAL;
    }
    if (mode != 0 && mode != 1) {
        set_err("%s: mode must be 0 (sum) or 1 (max), got %d", who, (int)mode);
        return AS_EINVAL;
    }
    for (int64_t t = 0; weights && t < j; ++t)
        if (!std::isfinite(weights[t])) {
            set_err("%s: weights[%lld] must be finite", who, (long long)t);
            return AS_EINVAL;
        }
    AS_TRY(own_subset(who, sp, sub));
    AS_TRY(subset_checks(who, sp, gr, d, &tau, 1));
    try {
        if (weights) wts.assign(weights, weights + j);
        else wts.assign((size_t)j, 1.0 / (double)j);
    } catch (const std::bad_alloc&) {
        set_err("%s: out of host memory for %lld weights", who, (long long)j);
        return AS_ENOMEM;
    }
    calls->fetch_add(1, std::memory_order_relaxed);
    AS_TRY(batch_lambda_step(who, sp, gr, queries, j, d, tau, steps, lq, st, out_lambda_q, out_status));
    int64_t served = 0;
    for (int64_t t = 0; t < j; ++t) served += st[t] == AS_EZEROLAMBDA ? 0 : 1;
    if (served == 0 || (served < j && !skip_zero)) {
        set_err("The lambdas are zero, check the magnitude of items and eps.");
        return AS_EZEROLAMBDA;
    }
    return AS_OK;
}
as_status fused_sink_chunk(void* ctx, SubsetWork*, int64_t i0, int64_t nb, const double* scores, int64_t ld) {
    return fused_chunk((FusedCall*)ctx, i0, nb, scores, ld);
}
// the j score rows of the work's m ids, chunk by chunk, folded into the work's accumulator; the stream is left busy at most with
// what the caller queues behind (the selection, or the copy of the accumulator)
as_status fused_fold(const as_space* sp, SubsetWork* w, int64_t m, const double* queries, int64_t j, double tau, const std::vector<double>& wts,
                     const std::vector<double>& lq, const std::vector<int32_t>& st, int32_t mode, FusedCall* call) {
    AS_TRY(fused_begin(w, m, j, wts.data(), st.data(), mode, call));
    const SubsetChunkSink sink{fused_sink_chunk, call};
    return subset_batch_run(sp, w, m, queries, j, lq.data(), st.data(), tau, 0, 0, nullptr, nullptr, nullptr, nullptr, &sink);
}
void fused_counts_add(const as_space* sp, const FusedCall& call) {
    sp->fused_count[1].fetch_add(call.launches, std::memory_order_relaxed);
    sp->fused_count[2].fetch_add(call.folded, std::memory_order_relaxed);
    sp->fused_us.store(call.us, std::memory_order_relaxed);
}
}  // namespace

as_status as_search_fused(const as_space* sp, const as_graph* gr, const double* queries, int64_t j, int64_t d, double tau, const double* weights,
                          int32_t mode, int32_t skip_zero, const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len,
                          double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || !queries || !out_len || ((!sub || sub->m > 0) && (!out_idx || !out_score))) {
        set_err("as_search_fused: null argument");
        return AS_EINVAL;
    }
    *out_len = 0;
    std::vector<double> wts, lq;
    std::vector<int32_t> st;
    AS_TRY(fused_prepare("as_search_fused", sp, gr, queries, j, d, tau, weights, mode, skip_zero, sub, out_lambda_q, out_status, wts, lq, st,
                         &sp->fused_count[0], &sp->fused_count[3]));
    if (sub && sub->m == 0) return AS_OK;
    const Candidates c("as_search_fused", sp, sub);
    AS_TRY(c.status);
    FusedCall call;
    as_status s = fused_fold(sp, c.w, c.m, queries, j, tau, wts, lq, st, mode, &call);
    if (s == AS_OK) s = subset_select_from(c.w, fused_acc(c.w), c.m, hits_bound(sp, gr, c.m), out_idx, out_score, out_len);
    s = s == AS_OK ? fused_end(&call) : c.fail(s);
    fused_counts_add(sp, call);
    return s;
}

as_status as_score_fused(const as_space* sp, const as_graph* gr, const double* queries, int64_t j, int64_t d, double tau, const double* weights,
                         int32_t mode, int32_t skip_zero, const int64_t* ids_host, int64_t m, double* out_scores, double* out_lambda_q,
                         int32_t* out_status) {
    if (!sp || !gr || !queries || m < 0 || (m > 0 && (!ids_host || !out_scores))) {
        set_err("as_score_fused: null argument");
        return AS_EINVAL;
    }
    AS_TRY(ids_in_range("as_score_fused", sp, ids_host, m));
    std::vector<double> wts, lq;
    std::vector<int32_t> st;
    AS_TRY(fused_prepare("as_score_fused", sp, gr, queries, j, d, tau, weights, mode, skip_zero, nullptr, out_lambda_q, out_status, wts, lq, st,
                         &sp->fused_count[0], &sp->fused_count[3]));
    if (m == 0) return AS_OK;
    std::vector<int32_t> ids;
    AS_TRY(checked_ids("as_score_fused", ids_host, m, ids));
    const Candidates c("as_score_fused", sp, ids.data(), m);
    AS_TRY(c.status);
    SubsetWork* w = c.w;
    FusedCall call;
    as_status s = fused_fold(sp, w, m, queries, j, tau, wts, lq, st, mode, &call);
    if (s == AS_OK && hipMemcpyAsync(out_scores, fused_acc(w), sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, w->stream) != hipSuccess) {
        set_err("as_score_fused: the copy of the scores failed");
        s = AS_EHIP;
    }
    if (hipStreamSynchronize(w->stream) != hipSuccess && s == AS_OK) {
        set_err("as_score_fused: the wait for the stream failed");
        s = AS_EHIP;
    }
    if (s == AS_OK) s = fused_end(&call);
    fused_counts_add(sp, call);
    return s;
}

as_status as_fused_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_fused_counters", sp, out, n, sp ? sp->fused_count : nullptr, 4);
}
double as_fused_kernel_us(const as_space* sp) { return sp ? sp->fused_us.load(std::memory_order_relaxed) : 0.0; }

// ---------------------------------------------------------------- batched fused search (extension; as_fused.hip)
namespace {
// b >= 1 needs; offsets [b + 1] start at 0, increase strictly (no empty need) and end at nv: looked at before any handle is
static as_status fused_batch_offsets(const char* who, const int64_t* offsets, int64_t b, int64_t nv) {
    if (b < 1) {
        set_err("%s: b must be >= 1, got %lld", who, (long long)b);
        return AS_EINVAL;
    }
    if (offsets[0] != 0 || offsets[b] != nv) {
        set_err("%s: offsets must start at 0 and end at nv = %lld, got %lld .. %lld", who, (long long)nv, (long long)offsets[0], (long long)offsets[b]);
        return AS_EINVAL;
    }
    for (int64_t y = 0; y < b; ++y)
        if (offsets[y + 1] <= offsets[y]) {
            set_err("%s: offsets must increase strictly (need %lld is empty or runs backwards)", who, (long long)y);
            return AS_EINVAL;
        }
    return AS_OK;
}
// What both forms refuse before anything is launched, then lambda_q and the status of every vector from ONE as_search_batch call
// over the nv vectors, then S15's zero-lambda rule: `nst` is the status per need.  `wts`: the caller's weights, or 1/J_b each.
// calls, needs, steps: the family's counters of calls that passed their checks, of their needs and of lambda_q steps.
struct FusedBatchArgs {
    std::vector<double> wts, lq;
    std::vector<int32_t> st, nst;
    bool any = false;   // a need is served
};
as_status fused_batch_prepare(const char* who, const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b,
                              int64_t d, double tau, const double* weights, int32_t mode, int32_t skip_zero, const as_subset* sub,
                              double* out_lambda_q, int32_t* out_status, FusedBatchArgs& a, std::atomic<int64_t>* calls,
                              std::atomic<int64_t>* needs, std::atomic<int64_t>* steps) {
    const int64_t nv = offsets[b];
    if (mode != 0 && mode != 1) {
        set_err("%s: mode must be 0 (sum) or 1 (max), got %d", who, (int)mode);
        return AS_EINVAL;
    }
    for (int64_t t = 0; weights && t < nv; ++t)
        if (!std::isfinite(weights[t])) {
            set_err("%s: weights[%lld] must be finite", who, (long long)t);
            return AS_EINVAL;
        }
    AS_TRY(own_subset(who, sp, sub));
    AS_TRY(subset_checks(who, sp, gr, d, &tau, 1));
    try {
        if (weights) a.wts.assign(weights, weights + nv);
        else {
            a.wts.resize((size_t)nv);
            for (int64_t y = 0; y < b; ++y)
                for (int64_t t = offsets[y]; t < offsets[y + 1]; ++t) a.wts[(size_t)t] = 1.0 / (double)(offsets[y + 1] - offsets[y]);
        }
        a.nst.assign((size_t)b, 0);
    } catch (const std::bad_alloc&) {
        set_err("%s: out of host memory for %lld weights", who, (long long)nv);
        return AS_ENOMEM;
    }
    calls->fetch_add(1, std::memory_order_relaxed);
    needs->fetch_add(b, std::memory_order_relaxed);
    AS_TRY(batch_lambda_step(who, sp, gr, queries, nv, d, tau, steps, a.lq, a.st, out_lambda_q, nullptr));
    bool refused = false;
    for (int64_t y = 0; y < b; ++y) {
        int64_t served = 0;
        for (int64_t t = offsets[y]; t < offsets[y + 1]; ++t) served += a.st[(size_t)t] == AS_EZEROLAMBDA ? 0 : 1;
        const bool zero = skip_zero ? served == 0 : served < offsets[y + 1] - offsets[y];
        a.nst[(size_t)y] = zero ? AS_EZEROLAMBDA : 0;
        if (out_status) out_status[y] = a.nst[(size_t)y];
        a.any = a.any || !zero;
        refused = refused || (zero && !skip_zero);
    }
    if (refused) {
        set_err("The lambdas are zero, check the magnitude of items and eps.");
        return AS_EZEROLAMBDA;
    }
    return AS_OK;
}
as_status fused_batch_sink_chunk(void* ctx, SubsetWork*, int64_t i0, int64_t nb, const double* scores, int64_t ld) {
    return fused_batch_chunk((FusedBatchCall*)ctx, i0, nb, scores, ld);
}
// needs g0 .. g0 + gn - 1 (one of them served): their slice of the vectors scored chunk by chunk, every chunk folded into the
// group's accumulator rows; the stream is left busy at most with the last fold
as_status fused_batch_fold_group(const as_space* sp, SubsetWork* w, int64_t m, const double* queries, const int64_t* offsets, int64_t g0, int64_t gn,
                                 double tau, const FusedBatchArgs& a, FusedBatchCall* call) {
    const int64_t v0 = offsets[g0], v1 = offsets[g0 + gn];
    fused_batch_group(call, g0, gn);
    const SubsetChunkSink sink{fused_batch_sink_chunk, call};
    return subset_batch_run(sp, w, m, queries + v0 * sp->d, v1 - v0, a.lq.data() + v0, a.st.data() + v0, tau, 0, 0, nullptr, nullptr, nullptr, nullptr,
                            &sink);
}
bool fused_batch_group_served(const FusedBatchArgs& a, int64_t g0, int64_t gn) {
    for (int64_t t = 0; t < gn; ++t)
        if (a.nst[(size_t)(g0 + t)] == 0) return true;
    return false;
}
void fused_batch_counts_add(const as_space* sp, const FusedBatchCall& call) {
    sp->fused_batch_count[2].fetch_add(call.launches, std::memory_order_relaxed);
    sp->fused_batch_count[3].fetch_add(call.folded, std::memory_order_relaxed);
    sp->fused_batch_count[5].fetch_add(call.groups, std::memory_order_relaxed);
    sp->fused_batch_us.store(call.us, std::memory_order_relaxed);
}
}  // namespace

as_status as_search_fused_batch(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                                int64_t d, double tau, const double* weights, int32_t mode, int32_t skip_zero, const as_subset* sub,
                                int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || !queries || !offsets || !out_len || ((!sub || sub->m > 0) && (!out_idx || !out_score))) {
        set_err("as_search_fused_batch: null argument");
        return AS_EINVAL;
    }
    AS_TRY(fused_batch_offsets("as_search_fused_batch", offsets, b, nv));
    for (int64_t y = 0; y < b; ++y) out_len[y] = 0;
    FusedBatchArgs a;
    AS_TRY(fused_batch_prepare("as_search_fused_batch", sp, gr, queries, offsets, b, d, tau, weights, mode, skip_zero, sub, out_lambda_q,
                               out_status, a, &sp->fused_batch_count[0], &sp->fused_batch_count[1], &sp->fused_batch_count[4]));
    if ((sub && sub->m == 0) || !a.any) return AS_OK;
    const Candidates c("as_search_fused_batch", sp, sub);
    AS_TRY(c.status);
    const int64_t kk = hits_bound(sp, gr, c.m), k = std::min<int64_t>(kk, SUBSET_TOPK);
    FusedBatchCall call;
    as_status s = fused_batch_begin(c.w, c.m, b, offsets, a.wts.data(), a.st.data(), mode, &call);
    for (int64_t g0 = 0; s == AS_OK && g0 < b; g0 += call.gmax) {
        const int64_t gn = std::min<int64_t>(call.gmax, b - g0);
        if (!fused_batch_group_served(a, g0, gn)) continue;
        s = fused_batch_fold_group(sp, c.w, c.m, queries, offsets, g0, gn, tau, a, &call);
        if (s == AS_OK) s = subset_select_rows_from(c.w, fused_acc(c.w), c.w->ids, c.m, c.m, k, gn);   // -> c.w->out[t]; waits
        for (int64_t t = 0; s == AS_OK && t < gn; ++t) {
            const int64_t y = g0 + t;
            if (a.nst[(size_t)y] == 0) s = subset_list_out(c.w->out + t, k, out_idx + y * kk, out_score + y * kk, out_len + y);
        }
    }
    if (s == AS_OK) s = fused_batch_end(&call);
    else {
        (void)c.fail(s);
        for (int64_t y = 0; y < b; ++y) out_len[y] = 0;
    }
    fused_batch_counts_add(sp, call);
    return s;
}

as_status as_score_fused_batch(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                               int64_t d, double tau, const double* weights, int32_t mode, int32_t skip_zero, const int64_t* ids_host, int64_t m,
                               double* out_scores, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || !queries || !offsets || m < 0 || (m > 0 && (!ids_host || !out_scores))) {
        set_err("as_score_fused_batch: null argument");
        return AS_EINVAL;
    }
    AS_TRY(fused_batch_offsets("as_score_fused_batch", offsets, b, nv));
    AS_TRY(ids_in_range("as_score_fused_batch", sp, ids_host, m));
    FusedBatchArgs a;
    AS_TRY(fused_batch_prepare("as_score_fused_batch", sp, gr, queries, offsets, b, d, tau, weights, mode, skip_zero, nullptr, out_lambda_q,
                               out_status, a, &sp->fused_batch_count[0], &sp->fused_batch_count[1], &sp->fused_batch_count[4]));
    if (m == 0) return AS_OK;
    // an unserved need's row: NaN
    const auto nan_rows = [&](int64_t g0, int64_t gn) {
        for (int64_t y = g0; y < g0 + gn; ++y)
            if (a.nst[(size_t)y] != 0) std::fill(out_scores + y * m, out_scores + (y + 1) * m, std::numeric_limits<double>::quiet_NaN());
    };
    if (!a.any) {
        nan_rows(0, b);
        return AS_OK;
    }
    std::vector<int32_t> ids;
    AS_TRY(checked_ids("as_score_fused_batch", ids_host, m, ids));
    const Candidates c("as_score_fused_batch", sp, ids.data(), m);
    AS_TRY(c.status);
    SubsetWork* w = c.w;
    FusedBatchCall call;
    as_status s = fused_batch_begin(w, m, b, offsets, a.wts.data(), a.st.data(), mode, &call);
    for (int64_t g0 = 0; s == AS_OK && g0 < b; g0 += call.gmax) {
        const int64_t gn = std::min<int64_t>(call.gmax, b - g0);
        if (fused_batch_group_served(a, g0, gn)) {
            s = fused_batch_fold_group(sp, w, m, queries, offsets, g0, gn, tau, a, &call);
            // the group's accumulator rows in one copy (an unserved need's row holds no answer: overwritten below)
            if (s == AS_OK && hipMemcpyAsync(out_scores + g0 * m, fused_acc(w), sizeof(double) * (size_t)(gn * m), hipMemcpyDeviceToHost, w->stream) !=
                                  hipSuccess) {
                set_err("as_score_fused_batch: the copy of the scores failed");
                s = AS_EHIP;
            }
            if (hipStreamSynchronize(w->stream) != hipSuccess && s == AS_OK) {
                set_err("as_score_fused_batch: the wait for the stream failed");
                s = AS_EHIP;
            }
        }
        if (s == AS_OK) nan_rows(g0, gn);
    }
    if (s == AS_OK) s = fused_batch_end(&call);
    fused_batch_counts_add(sp, call);
    return s;
}

as_status as_fused_batch_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_fused_batch_counters", sp, out, n, sp ? sp->fused_batch_count : nullptr, 6);
}
double as_fused_batch_kernel_us(const as_space* sp) { return sp ? sp->fused_batch_us.load(std::memory_order_relaxed) : 0.0; }

// ---------------------------------------------------------------- grouped search (extension; as_grouped.hip)
as_status as_groups_create(const as_space* sp, const int64_t* labels, int64_t n, as_groups** out) {
    if (!sp || !labels || !out) {
        set_err("as_groups_create: null argument");
        return AS_EINVAL;
    }
    *out = nullptr;
    if (n != sp->n) {
        set_err("as_groups_create: %lld labels for %lld items", (long long)n, (long long)sp->n);
        return AS_EINVAL;
    }
    as_groups* g = nullptr;
    try {
        g = new as_groups();
        g->labels.assign(labels, labels + n);
        std::sort(g->labels.begin(), g->labels.end());
        g->labels.erase(std::unique(g->labels.begin(), g->labels.end()), g->labels.end());
        g->dense.resize((size_t)n);
        g->size.assign(g->labels.size(), 0);
    } catch (const std::bad_alloc&) {
        delete g;
        set_err("as_groups_create: out of host memory for %lld labels", (long long)n);
        return AS_ENOMEM;
    }
    g->sp = sp;
    g->device = sp->device;
    g->n = n;
    g->count = (int64_t)g->labels.size();
    for (int64_t i = 0; i < n; ++i) {   // (group numbers fit 32 bits: space_new refuses n >= 2^31)
        const int32_t d = (int32_t)(std::lower_bound(g->labels.begin(), g->labels.end(), labels[i]) - g->labels.begin());
        g->dense[(size_t)i] = d;
        g->size[(size_t)d] += 1;
    }
    hipError_t e = hipSetDevice(sp->device);
    if (e == hipSuccess) e = hipMalloc((void**)&g->dense_dev, sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1));
    if (e == hipSuccess) e = hipMemcpy(g->dense_dev, g->dense.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_err("as_groups_create: the upload of %lld group numbers failed: %s", (long long)n, hipGetErrorString(e));
        as_groups_free(g);
        return e == hipErrorOutOfMemory ? AS_ENOMEM : AS_EHIP;
    }
    *out = g;
    return AS_OK;
}
int64_t as_groups_count(const as_groups* g) { return g ? g->count : 0; }
void as_groups_free(as_groups* g) {
    if (!g) return;
    if (g->dense_dev) {
        (void)hipSetDevice(g->device);
        (void)hipFree(g->dense_dev);
    }
    delete g;
}

namespace {
// what both forms refuse before anything is launched, the lambda_q step included
as_status grouped_checks(const char* who, const as_space* sp, const as_graph* gr, int64_t d, double tau, const as_groups* groups,
                         int64_t n_groups, int64_t per_group, const as_subset* sub) {
    if (n_groups < 1 || n_groups > SUBSET_TOPK) {
        set_err("%s: n_groups must be in [1, %d], got %lld", who, SUBSET_TOPK, (long long)n_groups);
        return AS_EINVAL;
    }
    if (per_group < 1 || per_group > GROUPED_MAX_PER_GROUP) {
        set_err("%s: per_group must be in [1, %d], got %lld", who, GROUPED_MAX_PER_GROUP, (long long)per_group);
        return AS_EINVAL;
    }
    if (groups->sp != sp) {
        set_err("%s: the groups were made for another space", who);
        return AS_EINVAL;
    }
    AS_TRY(own_subset(who, sp, sub));
    return subset_checks(who, sp, gr, d, &tau, 1);
}
void grouped_counts_add(const as_space* sp, const GroupedCall& call) {
    for (int i = 0; i < 5; ++i) sp->grouped_count[1 + i].fetch_add(call.counts[i], std::memory_order_relaxed);
    sp->grouped_us.store(call.us, std::memory_order_relaxed);
}
as_status grouped_sink_chunk(void* ctx, SubsetWork*, int64_t i0, int64_t nb, const double* scores, int64_t ld) {
    return grouped_rows((GroupedCall*)ctx, i0, nb, scores, ld);
}
}  // namespace

as_status as_search_grouped(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, const as_groups* groups,
                            int64_t n_groups, int64_t per_group, const as_subset* sub, int64_t* out_label, int64_t* out_count,
                            int64_t* out_idx, double* out_score, int64_t* out_ngroups, double* out_lambda_q) {
    if (!sp || !gr || !query || !groups || !out_label || !out_count || !out_idx || !out_score || !out_ngroups) {
        set_err("as_search_grouped: null argument");
        return AS_EINVAL;
    }
    *out_ngroups = 0;
    AS_TRY(grouped_checks("as_search_grouped", sp, gr, d, tau, groups, n_groups, per_group, sub));
    sp->grouped_count[0].fetch_add(1, std::memory_order_relaxed);
    double lq = 0.0;
    AS_TRY(lambda_step(sp, gr, query, d, tau, &sp->grouped_count[6], &lq, out_lambda_q));
    if (sub && sub->m == 0) return AS_OK;
    const Candidates c("as_search_grouped", sp, sub);
    AS_TRY(c.status);
    GroupedCall call;
    call.w = c.w; call.g = groups; call.m = c.m; call.n_groups = n_groups; call.per_group = per_group;
    call.out_label = out_label; call.out_count = out_count; call.out_idx = out_idx; call.out_score = out_score; call.out_ngroups = out_ngroups;
    as_status s = subset_score(sp, c.w, c.m, query, tau, lq);
    if (s == AS_OK) s = grouped_rows(&call, 0, 1, c.w->scores, c.m);
    if (c.fail(s) != AS_OK) *out_ngroups = 0;
    grouped_counts_add(sp, call);
    return s;
}

as_status as_search_grouped_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                  const as_groups* groups, int64_t n_groups, int64_t per_group, const as_subset* sub, int64_t* out_label,
                                  int64_t* out_count, int64_t* out_idx, double* out_score, int64_t* out_ngroups, double* out_lambda_q,
                                  int32_t* out_status) {
    if (!sp || !gr || !groups || b < 0 || (b > 0 && (!queries || !out_label || !out_count || !out_idx || !out_score || !out_ngroups))) {
        set_err("as_search_grouped_batch: null argument");
        return AS_EINVAL;
    }
    for (int64_t i = 0; i < b; ++i) out_ngroups[i] = 0;
    AS_TRY(grouped_checks("as_search_grouped_batch", sp, gr, d, tau, groups, n_groups, per_group, sub));
    sp->grouped_count[0].fetch_add(1, std::memory_order_relaxed);
    if (b == 0) return AS_OK;
    std::vector<double> lq;
    std::vector<int32_t> st;
    AS_TRY(batch_lambda_step("as_search_grouped_batch", sp, gr, queries, b, d, tau, &sp->grouped_count[6], lq, st, out_lambda_q, out_status));
    if (sub && sub->m == 0) return AS_OK;
    const Candidates c("as_search_grouped_batch", sp, sub);
    AS_TRY(c.status);
    GroupedCall call;
    call.w = c.w; call.g = groups; call.m = c.m; call.n_groups = n_groups; call.per_group = per_group; call.status = st.data();
    call.out_label = out_label; call.out_count = out_count; call.out_idx = out_idx; call.out_score = out_score; call.out_ngroups = out_ngroups;
    SubsetChunkSink sink{grouped_sink_chunk, &call};
    sink.row_bytes = grouped_row_bytes(groups, c.m, n_groups, per_group);
    const as_status s = c.fail(subset_batch_run(sp, c.w, c.m, queries, b, lq.data(), st.data(), tau, 0, 0, nullptr, nullptr, nullptr, nullptr, &sink));
    if (s != AS_OK)
        for (int64_t i = 0; i < b; ++i) out_ngroups[i] = 0;
    grouped_counts_add(sp, call);
    return s;
}

as_status as_grouped_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_grouped_counters", sp, out, n, sp ? sp->grouped_count : nullptr, 7);
}
double as_grouped_kernel_us(const as_space* sp) { return sp ? sp->grouped_us.load(std::memory_order_relaxed) : 0.0; }

// ---------------------------------------------------------------- late-interaction search (extension; as_maxsim.hip)
namespace {
// what both forms refuse before anything is launched and before the fused forms' own checks
as_status maxsim_checks(const char* who, const as_space* sp, const as_groups* groups) {
    if (groups->sp != sp) {
        set_err("%s: the groups were made for another space", who);
        return AS_EINVAL;
    }
    return AS_OK;
}
as_status maxsim_sink_chunk(void* ctx, SubsetWork*, int64_t i0, int64_t nb, const double* scores, int64_t ld) {
    return maxsim_chunk((MaxsimCall*)ctx, i0, nb, scores, ld);
}
// the j score rows of the work's m ids, chunk by chunk, turned into group maxima and folded into the work's accumulator; the
// stream is left busy at most with what the caller queues behind (the selection, or the copy of the accumulator)
as_status maxsim_fold(const as_space* sp, SubsetWork* w, int64_t m, const double* queries, int64_t j, double tau, const as_groups* groups,
                      const std::vector<double>& wts, const std::vector<double>& lq, const std::vector<int32_t>& st, MaxsimCall* call) {
    AS_TRY(maxsim_begin(w, groups, m, j, wts.data(), st.data(), call));
    SubsetChunkSink sink{maxsim_sink_chunk, call};
    sink.row_bytes = groups->count * (int64_t)sizeof(unsigned long long);
    return subset_batch_run(sp, w, m, queries, j, lq.data(), st.data(), tau, 0, 0, nullptr, nullptr, nullptr, nullptr, &sink);
}
void maxsim_counts_add(const as_space* sp, const MaxsimCall& call) {
    sp->maxsim_count[1].fetch_add(call.served, std::memory_order_relaxed);
    sp->maxsim_count[2].fetch_add(call.passa, std::memory_order_relaxed);
    sp->maxsim_count[3].fetch_add(call.atoms, std::memory_order_relaxed);
    sp->maxsim_count[4].fetch_add(call.folds, std::memory_order_relaxed);
    for (int t = 0; t < 2; ++t) sp->maxsim_us[t].store(call.us[t], std::memory_order_relaxed);
}
}  // namespace

as_status as_search_maxsim(const as_space* sp, const as_graph* gr, const double* queries, int64_t j, int64_t d, double tau, const double* weights,
                           int32_t skip_zero, const as_groups* groups, int64_t n_groups, const as_subset* sub, int64_t* out_label,
                           double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || !queries || !groups || !out_label || !out_score || !out_len) {
        set_err("as_search_maxsim: null argument");
        return AS_EINVAL;
    }
    *out_len = 0;
    if (n_groups < 1 || n_groups > SUBSET_TOPK) {
        set_err("as_search_maxsim: n_groups must be in [1, %d], got %lld", SUBSET_TOPK, (long long)n_groups);
        return AS_EINVAL;
    }
    AS_TRY(maxsim_checks("as_search_maxsim", sp, groups));
    std::vector<double> wts, lq;
    std::vector<int32_t> st;
    AS_TRY(fused_prepare("as_search_maxsim", sp, gr, queries, j, d, tau, weights, 0, skip_zero, sub, out_lambda_q, out_status, wts, lq, st,
                         &sp->maxsim_count[0], nullptr));
    if (sub && sub->m == 0) return AS_OK;
    const Candidates c("as_search_maxsim", sp, sub);
    AS_TRY(c.status);
    MaxsimCall call;
    int64_t grp[SUBSET_TOPK], len = 0;
    double sc[SUBSET_TOPK];
    as_status s = maxsim_fold(sp, c.w, c.m, queries, j, tau, groups, wts, lq, st, &call);
    if (s == AS_OK) s = maxsim_select(&call, std::min<int64_t>(n_groups, groups->count), grp, sc, &len);
    s = c.fail(s);
    maxsim_counts_add(sp, call);
    AS_TRY(s);
    // entries that came back NaN lie behind the last group that exists
    int64_t n = 0;
    for (; n < len && sc[n] == sc[n]; ++n) {
        if (grp[n] < 0 || grp[n] >= groups->count) {
            set_err("as_search_maxsim: the selection returned group %lld", (long long)grp[n]);
            return AS_EHIP;
        }
        out_label[n] = groups->labels[(size_t)grp[n]];
        out_score[n] = sc[n];
    }
    *out_len = n;
    return AS_OK;
}

as_status as_score_maxsim(const as_space* sp, const as_graph* gr, const double* queries, int64_t j, int64_t d, double tau, const double* weights,
                          int32_t skip_zero, const as_groups* groups, const as_subset* sub, const int64_t* labels, int64_t nl, double* out_scores,
                          double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || !queries || !groups || nl < 0 || (nl > 0 && (!labels || !out_scores))) {
        set_err("as_score_maxsim: null argument");
        return AS_EINVAL;
    }
    AS_TRY(maxsim_checks("as_score_maxsim", sp, groups));
    std::vector<int64_t> pos;   // the dense group number of every listed label
    try {
        pos.resize((size_t)nl);
    } catch (const std::bad_alloc&) {
        set_err("as_score_maxsim: out of host memory for %lld labels", (long long)nl);
        return AS_ENOMEM;
    }
    for (int64_t t = 0; t < nl; ++t) {
        const auto it = std::lower_bound(groups->labels.begin(), groups->labels.end(), labels[t]);
        if (it == groups->labels.end() || *it != labels[t]) {
            set_err("as_score_maxsim: label %lld is not one of the groups", (long long)labels[t]);
            return AS_EINVAL;
        }
        pos[(size_t)t] = it - groups->labels.begin();
    }
    std::vector<double> wts, lq, F;
    std::vector<int32_t> st;
    AS_TRY(fused_prepare("as_score_maxsim", sp, gr, queries, j, d, tau, weights, 0, skip_zero, sub, out_lambda_q, out_status, wts, lq, st,
                         &sp->maxsim_count[0], nullptr));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (nl == 0) return AS_OK;
    if (sub && sub->m == 0) {   // no item, no member
        for (int64_t t = 0; t < nl; ++t) out_scores[t] = nan;
        return AS_OK;
    }
    try {
        F.assign((size_t)groups->count, nan);
    } catch (const std::bad_alloc&) {
        set_err("as_score_maxsim: out of host memory for %lld groups", (long long)groups->count);
        return AS_ENOMEM;
    }
    const Candidates c("as_score_maxsim", sp, sub);
    AS_TRY(c.status);
    MaxsimCall call;
    as_status s = maxsim_fold(sp, c.w, c.m, queries, j, tau, groups, wts, lq, st, &call);
    if (s == AS_OK) s = maxsim_scores(&call, F.data());
    s = c.fail(s);
    maxsim_counts_add(sp, call);
    AS_TRY(s);
    for (int64_t t = 0; t < nl; ++t) out_scores[t] = F[(size_t)pos[(size_t)t]];
    return AS_OK;
}

as_status as_maxsim_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_maxsim_counters", sp, out, n, sp ? sp->maxsim_count : nullptr, 5);
}
double as_maxsim_kernel_us(const as_space* sp, int32_t part) {
    if (!sp || part < 0 || part > 2) return 0.0;
    const double a = sp->maxsim_us[0].load(std::memory_order_relaxed), f = sp->maxsim_us[1].load(std::memory_order_relaxed);
    return part == 0 ? a + f : (part == 1 ? a : f);
}

// ---------------------------------------------------------------- batched late-interaction search (extension; as_maxsim.hip)
namespace {
as_status maxsim_batch_sink_chunk(void* ctx, SubsetWork*, int64_t i0, int64_t nb, const double* scores, int64_t ld) {
    return maxsim_batch_chunk((MaxsimBatchCall*)ctx, i0, nb, scores, ld);
}
// needs g0 .. g0 + gn - 1 (one of them served): their slice of the vectors scored chunk by chunk, every chunk turned into group
// maxima and folded into the group's accumulator rows; the stream is left busy at most with the last fold
as_status maxsim_batch_fold_group(const as_space* sp, SubsetWork* w, int64_t m, const double* queries, const int64_t* offsets, int64_t g0, int64_t gn,
                                  double tau, const as_groups* groups, const FusedBatchArgs& a, MaxsimBatchCall* call) {
    const int64_t v0 = offsets[g0], v1 = offsets[g0 + gn];
    maxsim_batch_group(call, g0, gn);
    SubsetChunkSink sink{maxsim_batch_sink_chunk, call};
    sink.row_bytes = groups->count * (int64_t)sizeof(unsigned long long);
    return subset_batch_run(sp, w, m, queries + v0 * sp->d, v1 - v0, a.lq.data() + v0, a.st.data() + v0, tau, 0, 0, nullptr, nullptr, nullptr, nullptr,
                            &sink);
}
void maxsim_batch_counts_add(const as_space* sp, const MaxsimBatchCall& call) {
    sp->maxsim_batch_count[2].fetch_add(call.served, std::memory_order_relaxed);
    sp->maxsim_batch_count[3].fetch_add(call.passa, std::memory_order_relaxed);
    sp->maxsim_batch_count[4].fetch_add(call.atoms, std::memory_order_relaxed);
    sp->maxsim_batch_count[5].fetch_add(call.folds, std::memory_order_relaxed);
    sp->maxsim_batch_count[7].fetch_add(call.groups, std::memory_order_relaxed);
    for (int t = 0; t < 2; ++t) sp->maxsim_batch_us[t].store(call.us[t], std::memory_order_relaxed);
}
}  // namespace

as_status as_search_maxsim_batch(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                                 int64_t d, double tau, const double* weights, int32_t skip_zero, const as_groups* groups, int64_t n_groups,
                                 const as_subset* sub, int64_t* out_label, double* out_score, int64_t* out_len, double* out_lambda_q,
                                 int32_t* out_status) {
    if (!sp || !gr || !queries || !offsets || !groups || !out_label || !out_score || !out_len) {
        set_err("as_search_maxsim_batch: null argument");
        return AS_EINVAL;
    }
    AS_TRY(fused_batch_offsets("as_search_maxsim_batch", offsets, b, nv));
    for (int64_t y = 0; y < b; ++y) out_len[y] = 0;
    if (n_groups < 1 || n_groups > SUBSET_TOPK) {
        set_err("as_search_maxsim_batch: n_groups must be in [1, %d], got %lld", SUBSET_TOPK, (long long)n_groups);
        return AS_EINVAL;
    }
    AS_TRY(maxsim_checks("as_search_maxsim_batch", sp, groups));
    FusedBatchArgs a;
    AS_TRY(fused_batch_prepare("as_search_maxsim_batch", sp, gr, queries, offsets, b, d, tau, weights, 0, skip_zero, sub, out_lambda_q, out_status,
                               a, &sp->maxsim_batch_count[0], &sp->maxsim_batch_count[1], &sp->maxsim_batch_count[6]));
    if ((sub && sub->m == 0) || !a.any || groups->count <= 0) return AS_OK;
    const Candidates c("as_search_maxsim_batch", sp, sub);
    AS_TRY(c.status);
    const int64_t k = std::min<int64_t>(n_groups, groups->count);
    MaxsimBatchCall call;
    as_status s = maxsim_batch_begin(c.w, groups, c.m, b, offsets, a.wts.data(), a.st.data(), &call);
    for (int64_t g0 = 0; s == AS_OK && g0 < b; g0 += call.gmax) {
        const int64_t gn = std::min<int64_t>(call.gmax, b - g0);
        if (!fused_batch_group_served(a, g0, gn)) continue;
        s = maxsim_batch_fold_group(sp, c.w, c.m, queries, offsets, g0, gn, tau, groups, a, &call);
        if (s == AS_OK) s = maxsim_batch_select(&call, k);   // -> c.w->out[t]; waits
        for (int64_t t = 0; s == AS_OK && t < gn; ++t) {
            const int64_t y = g0 + t;
            if (a.nst[(size_t)y] != 0) continue;
            const SubsetOut* o = c.w->out + t;
            if (o->len != k) {
                set_err("as_search_maxsim_batch: the selection returned %lld of %lld entries", (long long)o->len, (long long)k);
                s = AS_EHIP;
                break;
            }
            // entries that came back NaN lie behind the last group that exists
            int64_t n = 0;
            for (; n < k && o->score[n] == o->score[n]; ++n) {
                if (o->idx[n] < 0 || o->idx[n] >= groups->count) {
                    set_err("as_search_maxsim_batch: the selection returned group %lld", (long long)o->idx[n]);
                    s = AS_EHIP;
                    break;
                }
                out_label[y * n_groups + n] = groups->labels[(size_t)o->idx[n]];
                out_score[y * n_groups + n] = o->score[n];
            }
            if (s == AS_OK) out_len[y] = n;
        }
    }
    if (s == AS_OK) s = maxsim_batch_end(&call);
    if (s != AS_OK) {
        (void)c.fail(s);
        for (int64_t y = 0; y < b; ++y) out_len[y] = 0;
    }
    maxsim_batch_counts_add(sp, call);
    return s;
}

as_status as_score_maxsim_batch(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                                int64_t d, double tau, const double* weights, int32_t skip_zero, const as_groups* groups, const as_subset* sub,
                                const int64_t* labels, int64_t nl, double* out_scores, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || !queries || !offsets || !groups || nl < 0 || (nl > 0 && (!labels || !out_scores))) {
        set_err("as_score_maxsim_batch: null argument");
        return AS_EINVAL;
    }
    AS_TRY(fused_batch_offsets("as_score_maxsim_batch", offsets, b, nv));
    AS_TRY(maxsim_checks("as_score_maxsim_batch", sp, groups));
    std::vector<int32_t> pos;   // the dense group number of every listed label (group numbers fit 32 bits: as_groups_create)
    try {
        pos.resize((size_t)nl);
    } catch (const std::bad_alloc&) {
        set_err("as_score_maxsim_batch: out of host memory for %lld labels", (long long)nl);
        return AS_ENOMEM;
    }
    for (int64_t t = 0; t < nl; ++t) {
        const auto it = std::lower_bound(groups->labels.begin(), groups->labels.end(), labels[t]);
        if (it == groups->labels.end() || *it != labels[t]) {
            set_err("as_score_maxsim_batch: label %lld is not one of the groups", (long long)labels[t]);
            return AS_EINVAL;
        }
        pos[(size_t)t] = (int32_t)(it - groups->labels.begin());
    }
    FusedBatchArgs a;
    AS_TRY(fused_batch_prepare("as_score_maxsim_batch", sp, gr, queries, offsets, b, d, tau, weights, 0, skip_zero, sub, out_lambda_q, out_status, a,
                               &sp->maxsim_batch_count[0], &sp->maxsim_batch_count[1], &sp->maxsim_batch_count[6]));
    if (nl == 0) return AS_OK;
    // an unserved need's row: NaN
    const auto nan_rows = [&](int64_t g0, int64_t gn, bool all) {
        for (int64_t y = g0; y < g0 + gn; ++y)
            if (all || a.nst[(size_t)y] != 0) std::fill(out_scores + y * nl, out_scores + (y + 1) * nl, std::numeric_limits<double>::quiet_NaN());
    };
    if ((sub && sub->m == 0) || !a.any) {   // no item, no member; or no need to serve
        nan_rows(0, b, true);
        return AS_OK;
    }
    const Candidates c("as_score_maxsim_batch", sp, sub);
    AS_TRY(c.status);
    MaxsimBatchCall call;
    as_status s = maxsim_batch_begin(c.w, groups, c.m, b, offsets, a.wts.data(), a.st.data(), &call);
    if (s == AS_OK) s = maxsim_batch_labels(&call, pos.data(), nl);
    for (int64_t g0 = 0; s == AS_OK && g0 < b; g0 += call.gmax) {
        const int64_t gn = std::min<int64_t>(call.gmax, b - g0);
        if (fused_batch_group_served(a, g0, gn)) {
            s = maxsim_batch_fold_group(sp, c.w, c.m, queries, offsets, g0, gn, tau, groups, a, &call);
            // the listed F of the group's needs in one copy (an unserved need's row holds no answer: overwritten below)
            if (s == AS_OK) s = maxsim_batch_pick(&call, out_scores + g0 * nl);
        }
    }
    if (s == AS_OK) s = maxsim_batch_end(&call);   // waits
    s = c.fail(s);
    if (s == AS_OK) nan_rows(0, b, false);
    maxsim_batch_counts_add(sp, call);
    return s;
}

as_status as_maxsim_batch_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_maxsim_batch_counters", sp, out, n, sp ? sp->maxsim_batch_count : nullptr, 8);
}
double as_maxsim_batch_kernel_us(const as_space* sp, int32_t part) {
    if (!sp || part < 0 || part > 2) return 0.0;
    const double a = sp->maxsim_batch_us[0].load(std::memory_order_relaxed), f = sp->maxsim_batch_us[1].load(std::memory_order_relaxed);
    return part == 0 ? a + f : (part == 1 ? a : f);
}

// ---------------------------------------------------------------- late-interaction re-ranking of per-need candidate documents (extension; as_maxsim_lists.hip)
static int64_t host_ns_since(std::chrono::steady_clock::time_point t0);
namespace {
// The documents of both forms, checked before the lambda_q step and narrowed: need y's documents need_docs[y] .. need_docs[y + 1] - 1
// carry strictly ascending labels of the groups; document dd's entries doc_first[dd] .. doc_first[dd + 1] - 1 are ALL the members of
// its group, ascending.  gnum: the documents' dense group numbers, ids32: the entries.
as_status maxsim_lists_docs(const char* who, const as_space* sp, const as_groups* groups, int64_t b, const int64_t* need_docs,
                            const int64_t* doc_label, const int64_t* doc_first, const int64_t* ids, std::vector<int32_t>& gnum,
                            std::vector<int32_t>& ids32) {
    if (need_docs[0] != 0) {
        set_err("%s: need_docs[0] must be 0, got %lld", who, (long long)need_docs[0]);
        return AS_EINVAL;
    }
    for (int64_t y = 0; y < b; ++y)
        if (need_docs[y + 1] < need_docs[y]) {
            set_err("%s: need_docs must not decrease (need %lld)", who, (long long)y);
            return AS_EINVAL;
        }
    const int64_t nd = need_docs[b];
    if (nd == 0) return AS_OK;
    if (!doc_label || !doc_first || !ids) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    if (doc_first[0] != 0) {
        set_err("%s: doc_first[0] must be 0, got %lld", who, (long long)doc_first[0]);
        return AS_EINVAL;
    }
    try {
        gnum.resize((size_t)nd);
    } catch (const std::bad_alloc&) {
        set_err("%s: out of host memory for %lld documents", who, (long long)nd);
        return AS_ENOMEM;
    }
    for (int64_t y = 0; y < b; ++y)
        for (int64_t dd = need_docs[y]; dd < need_docs[y + 1]; ++dd) {
            const auto it = std::lower_bound(groups->labels.begin(), groups->labels.end(), doc_label[dd]);
            if (it == groups->labels.end() || *it != doc_label[dd]) {
                set_err("%s: label %lld is not one of the groups", who, (long long)doc_label[dd]);
                return AS_EINVAL;
            }
            if (dd > need_docs[y] && doc_label[dd] <= doc_label[dd - 1]) {
                set_err("%s: the labels of need %lld must increase strictly", who, (long long)y);
                return AS_EINVAL;
            }
            const int64_t g = it - groups->labels.begin();
            gnum[(size_t)dd] = (int32_t)g;
            if (doc_first[dd + 1] - doc_first[dd] != groups->size[(size_t)g]) {
                set_err("%s: document %lld of need %lld holds %lld entries, its group has %lld members", who, (long long)(dd - need_docs[y]),
                        (long long)y, (long long)(doc_first[dd + 1] - doc_first[dd]), (long long)groups->size[(size_t)g]);
                return AS_EINVAL;
            }
        }
    const int64_t ne = doc_first[nd];
    if (ne >= (int64_t)1 << 31) {
        set_err("%s: %lld entries exceed the supported maximum of 2^31 - 1 per call", who, (long long)ne);
        return AS_EUNSUPPORTED;
    }
    try {
        ids32.resize((size_t)ne);
    } catch (const std::bad_alloc&) {
        set_err("%s: out of host memory for %lld ids", who, (long long)ne);
        return AS_ENOMEM;
    }
    for (int64_t dd = 0; dd < nd; ++dd)
        for (int64_t e = doc_first[dd]; e < doc_first[dd + 1]; ++e) {
            const int64_t i = ids[e];
            if (i < 0 || i >= sp->n || groups->dense[(size_t)i] != gnum[(size_t)dd] || (e > doc_first[dd] && i <= ids[e - 1])) {
                set_err("%s: entry %lld (item %lld) is not the next member of the group with label %lld", who, (long long)e, (long long)i,
                        (long long)doc_label[dd]);
                return AS_EINVAL;
            }
            ids32[(size_t)e] = (int32_t)i;
        }
    return AS_OK;
}
// both forms behind their null checks: kk > 0 the search form, else the score form
as_status maxsim_lists_call(const char* who, const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b,
                            int64_t nv, int64_t d, double tau, const double* weights, int32_t skip_zero, const as_groups* groups, int64_t kk,
                            const int64_t* need_docs, const int64_t* doc_label, const int64_t* doc_first, const int64_t* ids, int64_t* out_label,
                            double* out_score, int64_t* out_len, double* out_F, double* out_lambda_q, int32_t* out_status) {
    AS_TRY(maxsim_checks(who, sp, groups));
    auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> gnum, ids32;
    AS_TRY(maxsim_lists_docs(who, sp, groups, b, need_docs, doc_label, doc_first, ids, gnum, ids32));
    int64_t host_ns = host_ns_since(t0);
    const int64_t nd = need_docs[b];
    FusedBatchArgs a;
    AS_TRY(fused_batch_prepare(who, sp, gr, queries, offsets, b, d, tau, weights, 0, skip_zero, nullptr, out_lambda_q, out_status, a,
                               &sp->maxsim_lists_count[0], &sp->maxsim_lists_count[1], &sp->maxsim_lists_count[7]));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (nd == 0 || !a.any) {   // no document at all, or no need to serve
        if (kk == 0) std::fill(out_F, out_F + nd, nan);
        sp->maxsim_lists_count[8].fetch_add(host_ns, std::memory_order_relaxed);
        return AS_OK;
    }
    MaxsimListsIn in;
    in.queries = queries; in.voffs = offsets; in.b = b; in.lq = a.lq.data(); in.vst = a.st.data(); in.nst = a.nst.data(); in.wts = a.wts.data();
    in.need_docs = need_docs; in.doc_first = doc_first; in.doc_gnum = gnum.data(); in.ids = ids32.data(); in.tau = tau; in.kk = kk;
    std::vector<int64_t> grp;
    if (kk > 0) {
        try {
            grp.resize((size_t)(b * kk));
        } catch (const std::bad_alloc&) {
            set_err("%s: out of host memory for %lld needs", who, (long long)b);
            return AS_ENOMEM;
        }
    }
    int64_t counts[6] = {0, 0, 0, 0, 0, 0};
    double us[3] = {0.0, 0.0, 0.0};
    as_status r;
    {
        std::lock_guard<std::mutex> lk(sp->lmu);
        r = hipSetDevice(sp->device) == hipSuccess ? AS_OK : AS_EHIP;
        if (r != AS_OK) set_err("%s: hipSetDevice failed", who);
        else r = maxsim_lists_run(sp, in, grp.data(), out_score, out_len, out_F, counts, us);
        for (int t = 0; t < 3; ++t) sp->maxsim_lists_us[t].store(us[t], std::memory_order_relaxed);
    }
    for (int c = 0; c < 5; ++c) sp->maxsim_lists_count[2 + c].fetch_add(counts[c], std::memory_order_relaxed);
    sp->maxsim_lists_count[8].fetch_add(host_ns + counts[5], std::memory_order_relaxed);
    if (r != AS_OK) {
        if (kk > 0)
            for (int64_t y = 0; y < b; ++y) out_len[y] = 0;
        return r;
    }
    if (kk > 0)
        for (int64_t y = 0; y < b; ++y)
            for (int64_t n = 0; n < out_len[y]; ++n) {
                const int64_t g = grp[(size_t)(y * kk + n)];
                if (g < 0 || g >= groups->count) {
                    set_err("%s: the selection returned group %lld", who, (long long)g);
                    for (int64_t z = 0; z < b; ++z) out_len[z] = 0;
                    return AS_EHIP;
                }
                out_label[y * kk + n] = groups->labels[(size_t)g];
            }
    return AS_OK;
}
}  // namespace

as_status as_search_maxsim_lists(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                                 int64_t d, double tau, const double* weights, int32_t skip_zero, const as_groups* groups, int64_t n_groups,
                                 const int64_t* need_docs, const int64_t* doc_label, const int64_t* doc_first, const int64_t* ids,
                                 int64_t* out_label, double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || !queries || !offsets || !groups || !need_docs || !out_label || !out_score || !out_len) {
        set_err("as_search_maxsim_lists: null argument");
        return AS_EINVAL;
    }
    AS_TRY(fused_batch_offsets("as_search_maxsim_lists", offsets, b, nv));
    for (int64_t y = 0; y < b; ++y) out_len[y] = 0;
    if (n_groups < 1 || n_groups > SUBSET_TOPK) {
        set_err("as_search_maxsim_lists: n_groups must be in [1, %d], got %lld", SUBSET_TOPK, (long long)n_groups);
        return AS_EINVAL;
    }
    return maxsim_lists_call("as_search_maxsim_lists", sp, gr, queries, offsets, b, nv, d, tau, weights, skip_zero, groups, n_groups, need_docs,
                             doc_label, doc_first, ids, out_label, out_score, out_len, nullptr, out_lambda_q, out_status);
}

as_status as_score_maxsim_lists(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                                int64_t d, double tau, const double* weights, int32_t skip_zero, const as_groups* groups,
                                const int64_t* need_docs, const int64_t* doc_label, const int64_t* doc_first, const int64_t* ids,
                                double* out_scores, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || !queries || !offsets || !groups || !need_docs) {
        set_err("as_score_maxsim_lists: null argument");
        return AS_EINVAL;
    }
    AS_TRY(fused_batch_offsets("as_score_maxsim_lists", offsets, b, nv));
    if (need_docs[b] > 0 && !out_scores) {
        set_err("as_score_maxsim_lists: null argument");
        return AS_EINVAL;
    }
    return maxsim_lists_call("as_score_maxsim_lists", sp, gr, queries, offsets, b, nv, d, tau, weights, skip_zero, groups, 0, need_docs, doc_label,
                             doc_first, ids, nullptr, nullptr, nullptr, out_scores, out_lambda_q, out_status);
}

as_status as_maxsim_lists_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_maxsim_lists_counters", sp, out, n, sp ? sp->maxsim_lists_count : nullptr, 9);
}
double as_maxsim_lists_kernel_us(const as_space* sp, int32_t part) {
    if (!sp || part < 0 || part > 3) return 0.0;
    double u[3];
    for (int t = 0; t < 3; ++t) u[t] = sp->maxsim_lists_us[t].load(std::memory_order_relaxed);
    return part == 0 ? u[0] + u[1] + u[2] : u[part - 1];
}
as_status as_maxsim_lists_geometry(const as_space* sp, int64_t* out_tile, int64_t* out_segment) {
    if (!sp || !out_tile || !out_segment) {
        set_err("as_maxsim_lists_geometry: null argument");
        return AS_EINVAL;
    }
    *out_tile = maxsim_lists_tile(sp->dp);
    *out_segment = maxsim_lists_segment();
    return AS_OK;
}

// ---------------------------------------------------------------- diversified search (extension; as_diverse.hip)
// what both forms refuse before anything is launched, the pool step included
static as_status diverse_checks(const char* who, const as_space* sp, const as_graph* gr, int64_t d, double tau, int64_t n, double diversity,
                                const as_subset* sub) {
    if (n < 1) {
        set_err("%s: n must be >= 1, got %lld", who, (long long)n);
        return AS_EINVAL;
    }
    if (!(diversity >= 0.0 && diversity <= 1.0)) {
        set_err("%s: diversity must lie in [0, 1], got %g", who, diversity);
        return AS_EINVAL;
    }
    AS_TRY(own_subset(who, sp, sub));
    return subset_checks(who, sp, gr, d, &tau, 1);
}
static void diverse_counts_add(const as_space* sp, const int64_t* counts) {
    for (int i = 0; i < 3; ++i) sp->diverse_count[1 + i].fetch_add(counts[i], std::memory_order_relaxed);
}

as_status as_search_diverse(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, int64_t n, double diversity,
                            const as_subset* sub, int64_t* out_idx, double* out_score, double* out_margin, int64_t* out_len,
                            double* out_lambda_q) {
    if (!sp || !gr || !query || !out_idx || !out_score || !out_len) {
        set_err("as_search_diverse: null argument");
        return AS_EINVAL;
    }
    *out_len = 0;
    AS_TRY(diverse_checks("as_search_diverse", sp, gr, d, tau, n, diversity, sub));
    sp->diverse_count[0].fetch_add(1, std::memory_order_relaxed);
    // the pool: ONE ordinary search of the route, its hits in its order
    int64_t pidx[SUBSET_TOPK], plen = 0;
    double psc[SUBSET_TOPK];
    double lq = 0.0;
    sp->diverse_count[4].fetch_add(1, std::memory_order_relaxed);
    const as_status s = sub ? as_search_subset(sp, gr, query, d, tau, sub, pidx, psc, &plen, &lq)
                            : search_pooled(sp, gr, query, d, tau, pidx, psc, &plen, &lq);
    if (out_lambda_q) *out_lambda_q = lq;
    if (s != AS_OK) return s;
    if (plen <= 0) return AS_OK;
    int64_t counts[3] = {0, 0, 0};
    std::lock_guard<std::mutex> lk(sp->dmu);
    AS_HIP(hipSetDevice(sp->device));
    // (a stride of plen: the single form's outputs hold min(n, plen) entries)
    const as_status s2 = diverse_run(sp, pidx, psc, &plen, plen, 1, n, diversity, out_idx, out_score, out_margin, out_len, counts);
    diverse_counts_add(sp, counts);
    return s2;
}

as_status as_search_diverse_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau, int64_t n,
                                  double diversity, const as_subset* sub, int64_t* out_idx, double* out_score, double* out_margin,
                                  int64_t* out_len, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || b < 0 || (b > 0 && (!queries || !out_len))) {
        set_err("as_search_diverse_batch: null argument");
        return AS_EINVAL;
    }
    const int64_t kk = hits_bound(sp, gr, sub ? sub->m : sp->n);
    if (b > 0 && kk > 0 && (!out_idx || !out_score)) {
        set_err("as_search_diverse_batch: null argument");
        return AS_EINVAL;
    }
    for (int64_t i = 0; i < b; ++i) out_len[i] = 0;
    AS_TRY(diverse_checks("as_search_diverse_batch", sp, gr, d, tau, n, diversity, sub));
    sp->diverse_count[0].fetch_add(1, std::memory_order_relaxed);
    if (b == 0) return AS_OK;
    // the pools: ONE batched search of the route over all b queries, every list at stride kk
    const int64_t kks = std::max<int64_t>(kk, 1);
    std::vector<int64_t> pidx, plen;
    std::vector<double> psc, lq;
    std::vector<int32_t> st;
    try {
        pidx.resize((size_t)(b * kks));
        psc.resize((size_t)(b * kks));
        plen.assign((size_t)b, 0);
        lq.assign((size_t)b, 0.0);
        st.assign((size_t)b, 0);
    } catch (const std::bad_alloc&) {
        set_err("as_search_diverse_batch: out of host memory for %lld queries", (long long)b);
        return AS_ENOMEM;
    }
    sp->diverse_count[4].fetch_add(1, std::memory_order_relaxed);
    AS_TRY(sub ? as_search_subset_batch(sp, gr, queries, b, d, tau, sub, pidx.data(), psc.data(), plen.data(), lq.data(), st.data())
               : as_search_batch(sp, gr, queries, b, d, tau, pidx.data(), psc.data(), plen.data(), lq.data(), st.data()));
    for (int64_t i = 0; i < b; ++i) {
        if (out_lambda_q) out_lambda_q[i] = lq[i];
        if (out_status) out_status[i] = st[i];
        if (st[i] == AS_EZEROLAMBDA) plen[i] = 0;
    }
    if (kk == 0) return AS_OK;
    int64_t counts[3] = {0, 0, 0};
    std::lock_guard<std::mutex> lk(sp->dmu);
    AS_HIP(hipSetDevice(sp->device));
    const as_status s2 = diverse_run(sp, pidx.data(), psc.data(), plen.data(), kk, b, n, diversity, out_idx, out_score, out_margin, out_len, counts);
    diverse_counts_add(sp, counts);
    return s2;
}

as_status as_diverse_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_diverse_counters", sp, out, n, sp ? sp->diverse_count : nullptr, 5);
}
double as_diverse_kernel_us(const as_space* sp) {
    if (!sp) return 0.0;
    std::lock_guard<std::mutex> lk(sp->dmu);
    return diverse_kernel_us(sp->diverse_ws);
}

// ---------------------------------------------------------------- graph-diffusion search (extension; as_diffuse.hip)
static as_status lists_checks(const char* who, const as_space* sp, const int64_t* ids_host, const int64_t* offs, int64_t b);   // (below)
namespace {
// what a form runs behind its pool: `steps` steps of the recurrence (S19) or, solve set, the conjugate-gradient solve of its fixed
// point (S20; section 5.23) to `tol` within `max_iters` iterations, with the per-query outputs of the solve (each may be null)
struct DiffuseSpec {
    double alpha = 0.0;
    int64_t steps = 0;
    bool solve = false;
    double tol = 0.0;
    int64_t max_iters = 0;
    int32_t* out_iters = nullptr;
    double* out_residual = nullptr;
    int32_t* out_state = nullptr;
    static DiffuseSpec recurrence(double alpha, int64_t steps) {
        DiffuseSpec ds;
        ds.alpha = alpha; ds.steps = steps;
        return ds;
    }
    static DiffuseSpec fixed_point(double alpha, double tol, int64_t max_iters, int32_t* out_iters, double* out_residual, int32_t* out_state) {
        DiffuseSpec ds;
        ds.alpha = alpha; ds.solve = true; ds.tol = tol; ds.max_iters = max_iters;
        ds.out_iters = out_iters; ds.out_residual = out_residual; ds.out_state = out_state;
        return ds;
    }
    std::atomic<int64_t>* count(const as_space* sp) const { return solve ? sp->diffuse_solve_count : sp->diffuse_count; }
    void fill(DiffuseCall& dc) const {
        dc.alpha = alpha;
        dc.steps = steps;
        if (solve) {
            dc.tol = tol; dc.max_iters = max_iters; dc.out_iters = out_iters; dc.out_residual = out_residual; dc.out_state = out_state;
        }
    }
    // a query the solve does not reach (zero lambda_q, an empty answer): 0 iterations, residual NaN, not converged
    void clear_info(int64_t b) const {
        for (int64_t i = 0; solve && i < b; ++i) {
            if (out_iters) out_iters[i] = 0;
            if (out_residual) out_residual[i] = std::numeric_limits<double>::quiet_NaN();
            if (out_state) out_state[i] = 0;
        }
    }
};
// what every form refuses before anything is launched, the route's search included
as_status diffuse_param_checks(const char* who, const as_space* sp, const as_graph* gr, const DiffuseSpec& ds) {
    if (!(ds.alpha >= 0.0 && ds.alpha < 1.0)) {
        set_err("%s: alpha must lie in [0, 1), got %g", who, ds.alpha);
        return AS_EINVAL;
    }
    if (!ds.solve && (ds.steps < 0 || ds.steps > 64)) {
        set_err("%s: steps must lie in [0, 64], got %lld", who, (long long)ds.steps);
        return AS_EINVAL;
    }
    if (ds.solve && !(std::isfinite(ds.tol) && ds.tol > 0.0)) {
        set_err("%s: tol must be finite and > 0, got %g", who, ds.tol);
        return AS_EINVAL;
    }
    if (ds.solve && (ds.max_iters < 1 || ds.max_iters > 1024)) {
        set_err("%s: max_iters must lie in [1, 1024], got %lld", who, (long long)ds.max_iters);
        return AS_EINVAL;
    }
    if (gr->lambda_mode == AS_LAMBDA_FEATURE) {
        set_err("%s: a feature-mode graph (its Laplacian is over the columns) is not supported", who);
        return AS_EUNSUPPORTED;
    }
    return AS_OK;
}
// ... and, behind subset_checks (or graph_matches and the shard test of the raw form): the graph covers exactly the space's items
as_status diffuse_graph_checks(const char* who, const as_space* sp, const as_graph* gr) {
    if (gr->n != sp->n) {
        set_err("%s: the graph (%lld nodes) does not cover exactly the %lld items of the space", who, (long long)gr->n, (long long)sp->n);
        return AS_EINVAL;
    }
    return AS_OK;
}
as_status diffuse_checks(const char* who, const as_space* sp, const as_graph* gr, int64_t d, double tau, const DiffuseSpec& ds,
                         const as_subset* sub) {
    AS_TRY(diffuse_param_checks(who, sp, gr, ds));
    AS_TRY(own_subset(who, sp, sub));
    AS_TRY(subset_checks(who, sp, gr, d, &tau, 1));
    return diffuse_graph_checks(who, sp, gr);
}
// the seeds of S19 from b pools at stride kk: a pool entry whose score is not finite is left out
as_status diffuse_pool_seeds(const char* who, const int64_t* pidx, const double* psc, const int64_t* plen, int64_t kk, int64_t b,
                             std::vector<int64_t>& offs, std::vector<int64_t>& ids, std::vector<double>& vals) {
    try {
        offs.assign((size_t)b + 1, 0);
        for (int64_t i = 0; i < b; ++i) {
            for (int64_t p = 0; p < plen[i]; ++p)
                if (std::isfinite(psc[i * kk + p])) {
                    ids.push_back(pidx[i * kk + p]);
                    vals.push_back(psc[i * kk + p]);
                }
            offs[(size_t)i + 1] = (int64_t)ids.size();
        }
    } catch (const std::bad_alloc&) {
        set_err("%s: out of host memory for the seeds of %lld queries", who, (long long)b);
        return AS_ENOMEM;
    }
    return AS_OK;
}
// the recurrence and its output, under sp->fmu
as_status diffuse_locked(const char* who, const as_space* sp, const as_graph* gr, const DiffuseCall& dc) {
    int64_t counts[4] = {0, 0, 0, 0};   // (three of the recurrence, four of the solve)
    std::lock_guard<std::mutex> lk(sp->fmu);
    if (hipSetDevice(sp->device) != hipSuccess) {
        set_err("%s: hipSetDevice failed", who);
        return AS_EHIP;
    }
    const as_status s = diffuse_run(sp, gr, dc, counts);
    std::atomic<int64_t>* cnt = dc.max_iters > 0 ? sp->diffuse_solve_count : sp->diffuse_count;
    for (int i = 0; i < (dc.max_iters > 0 ? 4 : 3); ++i) cnt[2 + i].fetch_add(counts[i], std::memory_order_relaxed);
    return s;
}
}  // namespace

namespace {
as_status search_diffuse_impl(const char* who, const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau,
                              const DiffuseSpec& ds, const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len,
                              double* out_lambda_q) {
    if (!sp || !gr || !query || !out_len || ((!sub || sub->m > 0) && (!out_idx || !out_score))) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    *out_len = 0;
    AS_TRY(diffuse_checks(who, sp, gr, d, tau, ds, sub));
    ds.count(sp)[0].fetch_add(1, std::memory_order_relaxed);
    ds.clear_info(1);
    // the pool: ONE ordinary search of the route, its hits in its order
    int64_t pidx[SUBSET_TOPK], plen = 0;
    double psc[SUBSET_TOPK];
    double lq = 0.0;
    ds.count(sp)[1].fetch_add(1, std::memory_order_relaxed);
    const as_status s = sub ? as_search_subset(sp, gr, query, d, tau, sub, pidx, psc, &plen, &lq)
                            : search_pooled(sp, gr, query, d, tau, pidx, psc, &plen, &lq);
    if (out_lambda_q) *out_lambda_q = lq;
    if (s != AS_OK) return s;
    if (sub && sub->m == 0) return AS_OK;
    std::vector<int64_t> offs, ids;
    std::vector<double> vals;
    AS_TRY(diffuse_pool_seeds(who, pidx, psc, &plen, SUBSET_TOPK, 1, offs, ids, vals));
    const Candidates c(who, sp, sub);
    AS_TRY(c.status);
    DiffuseCall dc;
    dc.b = 1; dc.offs = offs.data(); dc.ids = ids.data(); dc.vals = vals.data(); ds.fill(dc);
    dc.sel = c.w; dc.pos_ids = c.w->ids; dc.m = c.m; dc.k = hits_bound(sp, gr, c.m); dc.stride = dc.k;
    dc.out_idx = out_idx; dc.out_score = out_score; dc.out_len = out_len;
    return c.fail(diffuse_locked(who, sp, gr, dc));
}

// the pools of a batched form (ONE batched search of the route over all b queries), as seeds; served[i] = 0: a zero lambda_q
as_status diffuse_batch_pools(const char* who, const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                              const DiffuseSpec& ds, const as_subset* sub, double* out_lambda_q, int32_t* out_status, std::vector<int64_t>& offs,
                              std::vector<int64_t>& ids, std::vector<double>& vals, std::vector<int32_t>& served) {
    const int64_t kks = std::max<int64_t>(hits_bound(sp, gr, sub ? sub->m : sp->n), 1);
    std::vector<int64_t> pidx, plen;
    std::vector<double> psc, lq;
    std::vector<int32_t> st;
    try {
        pidx.resize((size_t)(b * kks));
        psc.resize((size_t)(b * kks));
        plen.assign((size_t)b, 0);
        lq.assign((size_t)b, 0.0);
        st.assign((size_t)b, 0);
        served.assign((size_t)b, 1);
    } catch (const std::bad_alloc&) {
        set_err("%s: out of host memory for %lld queries", who, (long long)b);
        return AS_ENOMEM;
    }
    ds.count(sp)[1].fetch_add(1, std::memory_order_relaxed);
    AS_TRY(sub ? as_search_subset_batch(sp, gr, queries, b, d, tau, sub, pidx.data(), psc.data(), plen.data(), lq.data(), st.data())
               : as_search_batch(sp, gr, queries, b, d, tau, pidx.data(), psc.data(), plen.data(), lq.data(), st.data()));
    for (int64_t i = 0; i < b; ++i) {
        if (out_lambda_q) out_lambda_q[i] = lq[i];
        if (out_status) out_status[i] = st[i];
        if (st[i] == AS_EZEROLAMBDA) {
            plen[i] = 0;
            served[i] = 0;
        }
    }
    return diffuse_pool_seeds(who, pidx.data(), psc.data(), plen.data(), kks, b, offs, ids, vals);
}

as_status search_diffuse_batch_impl(const char* who, const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d,
                                    double tau, const DiffuseSpec& ds, const as_subset* sub, int64_t* out_idx, double* out_score,
                                    int64_t* out_len, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || b < 0 || (b > 0 && (!queries || !out_len))) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    const int64_t kk = hits_bound(sp, gr, sub ? sub->m : sp->n);
    if (b > 0 && kk > 0 && (!out_idx || !out_score)) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    for (int64_t i = 0; i < b; ++i) out_len[i] = 0;
    AS_TRY(diffuse_checks(who, sp, gr, d, tau, ds, sub));
    ds.count(sp)[0].fetch_add(1, std::memory_order_relaxed);
    ds.clear_info(b);
    if (b == 0) return AS_OK;
    std::vector<int64_t> offs, ids;
    std::vector<double> vals;
    std::vector<int32_t> served;
    AS_TRY(diffuse_batch_pools(who, sp, gr, queries, b, d, tau, ds, sub, out_lambda_q, out_status, offs, ids, vals, served));
    if (kk == 0) return AS_OK;
    const Candidates c(who, sp, sub);
    AS_TRY(c.status);
    DiffuseCall dc;
    dc.b = b; dc.offs = offs.data(); dc.ids = ids.data(); dc.vals = vals.data(); dc.served = served.data(); ds.fill(dc);
    dc.sel = c.w; dc.pos_ids = c.w->ids; dc.m = c.m; dc.k = kk; dc.stride = kk;
    dc.out_idx = out_idx; dc.out_score = out_score; dc.out_len = out_len;
    return c.fail(diffuse_locked(who, sp, gr, dc));
}

as_status score_diffuse_batch_impl(const char* who, const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d,
                                   double tau, const DiffuseSpec& ds, const int64_t* ids_host, int64_t m, double* out_scores,
                                   double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || b < 0 || m < 0 || (b > 0 && !queries) || (m > 0 && !ids_host) || (b > 0 && m > 0 && !out_scores)) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    AS_TRY(ids_in_range(who, sp, ids_host, m));
    AS_TRY(diffuse_checks(who, sp, gr, d, tau, ds, nullptr));
    std::vector<int32_t> ids32;
    AS_TRY(checked_ids(who, ids_host, m, ids32));
    ds.count(sp)[0].fetch_add(1, std::memory_order_relaxed);
    ds.clear_info(b);
    if (b == 0) return AS_OK;
    std::vector<int64_t> offs, ids;
    std::vector<double> vals;
    std::vector<int32_t> served;
    AS_TRY(diffuse_batch_pools(who, sp, gr, queries, b, d, tau, ds, nullptr, out_lambda_q, out_status, offs, ids, vals, served));
    if (m == 0) return AS_OK;
    for (int64_t i = 0; i < b; ++i)
        if (!served[(size_t)i])
            for (int64_t j = 0; j < m; ++j) out_scores[i * m + j] = std::numeric_limits<double>::quiet_NaN();
    DiffuseCall dc;
    dc.b = b; dc.offs = offs.data(); dc.ids = ids.data(); dc.vals = vals.data(); dc.served = served.data(); ds.fill(dc);
    dc.pick_ids = ids32.data(); dc.m = m; dc.out_rows = out_scores;
    return diffuse_locked(who, sp, gr, dc);
}

as_status diffuse_seeds_impl(const char* who, const as_space* sp, const as_graph* gr, const int64_t* ids_host, const double* values_host,
                             const int64_t* offsets_host, int64_t b, const DiffuseSpec& ds, double* out_f) {
    if (!sp || !gr || b < 0 || !offsets_host || (b > 0 && !out_f)) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    AS_TRY(diffuse_param_checks(who, sp, gr, ds));
    if (offsets_host[b] > 0 && (!ids_host || !values_host)) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    AS_TRY(lists_checks(who, sp, ids_host, offsets_host, b));   // the offsets, the total, every id
    for (int64_t e = 0; e < offsets_host[b]; ++e)
        if (!std::isfinite(values_host[e])) {
            set_err("%s: seed value %lld is not finite", who, (long long)e);
            return AS_EINVAL;
        }
    try {
        std::vector<int64_t> seen;
        for (int64_t i = 0; i < b; ++i) {
            seen.assign(ids_host + offsets_host[i], ids_host + offsets_host[i + 1]);
            std::sort(seen.begin(), seen.end());
            if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) {
                set_err("%s: the seed ids of query %lld are not distinct", who, (long long)i);
                return AS_EINVAL;
            }
        }
    } catch (const std::bad_alloc&) {
        set_err("%s: out of host memory for the seeds", who);
        return AS_ENOMEM;
    }
    AS_TRY(graph_matches(sp, gr, who));
    if (sp->row_offset != 0 || gr->ncols) {
        set_err("%s: a shard of a row-sharded index is not supported", who);
        return AS_EUNSUPPORTED;
    }
    AS_TRY(diffuse_graph_checks(who, sp, gr));
    ds.count(sp)[0].fetch_add(1, std::memory_order_relaxed);
    ds.clear_info(b);
    if (b == 0) return AS_OK;
    DiffuseCall dc;
    dc.b = b; dc.offs = offsets_host; dc.ids = ids_host; dc.vals = values_host; ds.fill(dc);
    dc.out_rows = out_f;
    return diffuse_locked(who, sp, gr, dc);
}
}  // namespace

as_status as_search_diffuse(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, double alpha, int64_t steps,
                            const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q) {
    return search_diffuse_impl("as_search_diffuse", sp, gr, query, d, tau, DiffuseSpec::recurrence(alpha, steps), sub, out_idx, out_score, out_len,
                               out_lambda_q);
}
as_status as_search_diffuse_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau, double alpha,
                                  int64_t steps, const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len,
                                  double* out_lambda_q, int32_t* out_status) {
    return search_diffuse_batch_impl("as_search_diffuse_batch", sp, gr, queries, b, d, tau, DiffuseSpec::recurrence(alpha, steps), sub, out_idx,
                                     out_score, out_len, out_lambda_q, out_status);
}
as_status as_score_diffuse_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau, double alpha,
                                 int64_t steps, const int64_t* ids_host, int64_t m, double* out_scores, double* out_lambda_q,
                                 int32_t* out_status) {
    return score_diffuse_batch_impl("as_score_diffuse_batch", sp, gr, queries, b, d, tau, DiffuseSpec::recurrence(alpha, steps), ids_host, m,
                                    out_scores, out_lambda_q, out_status);
}
as_status as_diffuse_seeds(const as_space* sp, const as_graph* gr, const int64_t* ids_host, const double* values_host,
                           const int64_t* offsets_host, int64_t b, double alpha, int64_t steps, double* out_f) {
    return diffuse_seeds_impl("as_diffuse_seeds", sp, gr, ids_host, values_host, offsets_host, b, DiffuseSpec::recurrence(alpha, steps), out_f);
}

// ---- fixed-point diffusion search (extension; as_diffuse_solve.hip): the forms above with the
// conjugate-gradient solve of the fixed point in place of `steps` steps
as_status as_search_diffuse_solve(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, double alpha, double tol,
                                  int64_t max_iters, const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len,
                                  double* out_lambda_q, int32_t* out_iters, double* out_residual, int32_t* out_state) {
    return search_diffuse_impl("as_search_diffuse_solve", sp, gr, query, d, tau,
                               DiffuseSpec::fixed_point(alpha, tol, max_iters, out_iters, out_residual, out_state), sub, out_idx, out_score, out_len,
                               out_lambda_q);
}
as_status as_search_diffuse_solve_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                        double alpha, double tol, int64_t max_iters, const as_subset* sub, int64_t* out_idx,
                                        double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status, int32_t* out_iters,
                                        double* out_residual, int32_t* out_state) {
    return search_diffuse_batch_impl("as_search_diffuse_solve_batch", sp, gr, queries, b, d, tau,
                                     DiffuseSpec::fixed_point(alpha, tol, max_iters, out_iters, out_residual, out_state), sub, out_idx, out_score, out_len,
                                     out_lambda_q, out_status);
}
as_status as_score_diffuse_solve_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                       double alpha, double tol, int64_t max_iters, const int64_t* ids_host, int64_t m, double* out_scores,
                                       double* out_lambda_q, int32_t* out_status, int32_t* out_iters, double* out_residual,
                                       int32_t* out_state) {
    return score_diffuse_batch_impl("as_score_diffuse_solve_batch", sp, gr, queries, b, d, tau,
                                    DiffuseSpec::fixed_point(alpha, tol, max_iters, out_iters, out_residual, out_state), ids_host, m, out_scores,
                                    out_lambda_q, out_status);
}
as_status as_diffuse_solve_seeds(const as_space* sp, const as_graph* gr, const int64_t* ids_host, const double* values_host,
                                 const int64_t* offsets_host, int64_t b, double alpha, double tol, int64_t max_iters, double* out_f,
                                 int32_t* out_iters, double* out_residual, int32_t* out_state) {
    return diffuse_seeds_impl("as_diffuse_solve_seeds", sp, gr, ids_host, values_host, offsets_host, b,
                              DiffuseSpec::fixed_point(alpha, tol, max_iters, out_iters, out_residual, out_state), out_f);
}
as_status as_diffuse_solve_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_diffuse_solve_counters", sp, out, n, sp ? sp->diffuse_solve_count : nullptr, 6);
}
double as_diffuse_solve_kernel_us(const as_space* sp, int32_t part) {
    if (!sp) return 0.0;
    std::lock_guard<std::mutex> lk(sp->fmu);
    return diffuse_solve_kernel_us(sp->diffuse_ws, part);
}

// ---- graph eigenpairs (extension; as_spectral.hip)
namespace {
// what as_graph_eigs and as_spectral_op refuse about the graph and the blocks, before anything is launched
as_status spectral_graph_checks(const char* who, const as_space* sp, const as_graph* gr, int64_t n, int C) {
    if (gr->lambda_mode == AS_LAMBDA_FEATURE) {
        set_err("%s: a feature-mode graph (its Laplacian is over the columns) is not supported", who);
        return AS_EUNSUPPORTED;
    }
    AS_TRY(graph_matches(sp, gr, who));
    if (sp->row_offset != 0 || gr->ncols) {
        set_err("%s: a shard of a row-sharded index is not supported", who);
        return AS_EUNSUPPORTED;
    }
    AS_TRY(diffuse_graph_checks(who, sp, gr));
    if (n < C) {
        set_err("%s: %lld rows are fewer than the %d columns of the block", who, (long long)n, C);
        return AS_EINVAL;
    }
    if (4 * (int64_t)sizeof(double) * n * C > spectral_budget()) {
        set_err("%s: four blocks of %lld x %d doubles exceed the \"spectral_mib\" budget of %lld MiB", who, (long long)n, C,
                (long long)(spectral_budget() >> 20));
        return AS_EINVAL;
    }
    return AS_OK;
}
}  // namespace

as_status as_graph_eigs(const as_space* sp, const as_graph* gr, int64_t m, double tol, int64_t max_iters, int64_t degree, int64_t seed,
                        double* out_values, double* out_vectors, double* out_residuals, int64_t* out_info) {
    const char* who = "as_graph_eigs";
    if (!sp || !gr || !out_values || !out_vectors || !out_residuals || !out_info) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    if (m < 1 || m > 48) {
        set_err("%s: m must lie in [1, 48], got %lld", who, (long long)m);
        return AS_EINVAL;
    }
    if (!(std::isfinite(tol) && tol > 0.0 && tol < 1.0)) {
        set_err("%s: tol must be finite and lie in (0, 1), got %g", who, tol);
        return AS_EINVAL;
    }
    if (max_iters < 1 || max_iters > 10000) {
        set_err("%s: max_iters must lie in [1, 10000], got %lld", who, (long long)max_iters);
        return AS_EINVAL;
    }
    if (degree < 1 || degree > 64) {
        set_err("%s: degree must lie in [1, 64], got %lld", who, (long long)degree);
        return AS_EINVAL;
    }
    if (seed < 0) {
        set_err("%s: seed must lie in [0, 2^63), got %lld", who, (long long)seed);
        return AS_EINVAL;
    }
    const int C = m <= 12 ? 16 : 64;
    AS_TRY(spectral_graph_checks(who, sp, gr, gr->n, C));
    sp->eigs_count[0].fetch_add(1, std::memory_order_relaxed);
    SpectralCall sc;
    sc.m = (int)m; sc.C = C; sc.tol = tol; sc.max_iters = max_iters; sc.degree = (int)degree; sc.seed = seed;
    sc.out_values = out_values; sc.out_vectors = out_vectors; sc.out_residuals = out_residuals; sc.out_info = out_info;
    int64_t counts[5] = {0, 0, 0, 0, 0};
    std::lock_guard<std::mutex> lk(sp->fmu);
    if (hipSetDevice(sp->device) != hipSuccess) {
        set_err("%s: hipSetDevice failed", who);
        return AS_EHIP;
    }
    const as_status s = spectral_eigs(sp, gr, sc, counts);
    for (int i = 0; i < 5; ++i) sp->eigs_count[1 + i].fetch_add(counts[i], std::memory_order_relaxed);
    return s;
}
as_status as_graph_eigs_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_graph_eigs_counters", sp, out, n, sp ? sp->eigs_count : nullptr, 6);
}
double as_graph_eigs_kernel_us(const as_space* sp, int32_t part) {
    if (!sp) return 0.0;
    std::lock_guard<std::mutex> lk(sp->fmu);
    return spectral_kernel_us(sp->diffuse_ws, part);
}
as_status as_spectral_op(const as_space* sp, const as_graph* gr, int32_t op, int64_t n, int32_t C, const double* a_host, const double* b_host,
                         const double* t_host, const double* coef, double* out_host) {
    const char* who = "as_spectral_op";
    if (!sp || !gr || !a_host || !out_host) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    if (op < AS_SPECTRAL_STEP || op > AS_SPECTRAL_COLNORM2 || (C != 16 && C != 64) || n < 1) {
        set_err("%s: op must be 0 .. 3, C 16 or 64 and n >= 1, got op %d, C %d, n %lld", who, (int)op, (int)C, (long long)n);
        return AS_EINVAL;
    }
    const bool step = op == AS_SPECTRAL_STEP;
    if ((step && (!coef || n != gr->n || (coef[2] != 0.0 && !b_host) || (coef[3] != 0.0 && !b_host))) ||
        ((op == AS_SPECTRAL_ROTATE || op == AS_SPECTRAL_COLNORM2) && !t_host) || (op == AS_SPECTRAL_COLNORM2 && !b_host)) {
        set_err("%s: op %d lacks an argument (the step: n is the graph's, W with g != 0)", who, (int)op);
        return AS_EINVAL;
    }
    AS_TRY(spectral_graph_checks(who, sp, gr, n, C));
    std::lock_guard<std::mutex> lk(sp->fmu);
    if (hipSetDevice(sp->device) != hipSuccess) {
        set_err("%s: hipSetDevice failed", who);
        return AS_EHIP;
    }
    return spectral_op(sp, gr, op, n, C, a_host, b_host, t_host, coef, out_host);
}
int32_t as_sym_eig_host(const double* a, int32_t n, double* w, double* v) { return sym_eig_host(a, n, w, v); }

// ---- connected components (extension; as_components.hip)
namespace {
// what both forms refuse about the graph, before anything is launched: what the raw diffusion form refuses
as_status components_graph_checks(const char* who, const as_space* sp, const as_graph* gr) {
    if (gr->lambda_mode == AS_LAMBDA_FEATURE) {
        set_err("%s: a feature-mode graph (its Laplacian is over the columns) is not supported", who);
        return AS_EUNSUPPORTED;
    }
    AS_TRY(graph_matches(sp, gr, who));
    if (sp->row_offset != 0 || gr->ncols) {
        set_err("%s: a shard of a row-sharded index is not supported", who);
        return AS_EUNSUPPORTED;
    }
    return diffuse_graph_checks(who, sp, gr);
}
// the call behind the checks: its counters, the lock of the diffusion forms, the run
as_status components_locked(const char* who, const as_space* sp, const as_graph* gr, const double* ts, int32_t nt, int32_t* labels_host,
                            as_components_info* info) {
    sp->components_count[0].fetch_add(1, std::memory_order_relaxed);
    sp->components_count[1].fetch_add(ts ? nt : 1, std::memory_order_relaxed);
    int64_t counts[3] = {0, 0, 0};
    std::lock_guard<std::mutex> lk(sp->fmu);
    if (hipSetDevice(sp->device) != hipSuccess) {
        set_err("%s: hipSetDevice failed", who);
        return AS_EHIP;
    }
    const as_status s = components_run(sp, gr, ts, nt, labels_host, info, counts);
    for (int i = 0; i < 3; ++i) sp->components_count[2 + i].fetch_add(counts[i], std::memory_order_relaxed);
    return s;
}
}  // namespace

as_status as_graph_components(const as_space* sp, const as_graph* gr, const double* max_dist, int32_t* labels_host, as_components_info* info) {
    const char* who = "as_graph_components";
    if (!sp || !gr || !labels_host) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    if (max_dist && std::isnan(*max_dist)) {
        set_err("%s: max_dist must not be a NaN", who);
        return AS_EINVAL;
    }
    AS_TRY(components_graph_checks(who, sp, gr));
    return components_locked(who, sp, gr, max_dist, 1, labels_host, info);
}
as_status as_graph_components_sweep(const as_space* sp, const as_graph* gr, const double* max_dists, int32_t nt, as_components_info* info) {
    const char* who = "as_graph_components_sweep";
    if (!sp || !gr || !max_dists || !info) {
        set_err("%s: null argument", who);
        return AS_EINVAL;
    }
    if (nt < 1 || nt > 64) {
        set_err("%s: the number of thresholds must lie in [1, 64], got %d", who, (int)nt);
        return AS_EINVAL;
    }
    for (int32_t i = 0; i < nt; ++i)
        if (std::isnan(max_dists[i])) {
            set_err("%s: max_dists[%d] must not be a NaN", who, (int)i);
            return AS_EINVAL;
        }
    AS_TRY(components_graph_checks(who, sp, gr));
    return components_locked(who, sp, gr, max_dists, nt, nullptr, info);
}
as_status as_components_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_components_counters", sp, out, n, sp ? sp->components_count : nullptr, 5);
}
double as_components_kernel_us(const as_space* sp, int32_t part) {
    if (!sp) return 0.0;
    std::lock_guard<std::mutex> lk(sp->fmu);
    return components_kernel_us(sp->diffuse_ws, part);
}

as_status as_diffuse_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_diffuse_counters", sp, out, n, sp ? sp->diffuse_count : nullptr, 5);
}
double as_diffuse_kernel_us(const as_space* sp) {
    if (!sp) return 0.0;
    std::lock_guard<std::mutex> lk(sp->fmu);
    return diffuse_kernel_us(sp->diffuse_ws);
}

// ---------------------------------------------------------------- per-query candidate lists (extension)
// What both forms check before anything is launched, the lambda_q step included: the offsets, the total, every id.
static as_status lists_checks(const char* who, const as_space* sp, const int64_t* ids_host, const int64_t* offs, int64_t b) {
    if (offs[0] != 0) {
        set_err("%s: offsets[0] must be 0, got %lld", who, (long long)offs[0]);
        return AS_EINVAL;
    }
    for (int64_t i = 0; i < b; ++i)
        if (offs[i + 1] < offs[i]) {
            set_err("%s: offsets must not decrease (offsets[%lld] = %lld after %lld)", who, (long long)(i + 1), (long long)offs[i + 1],
                    (long long)offs[i]);
            return AS_EINVAL;
        }
    if (offs[b] >= (int64_t)1 << 31) {
        set_err("%s: %lld ids exceed the supported maximum of 2^31 - 1 per call", who, (long long)offs[b]);
        return AS_EUNSUPPORTED;
    }
    for (int64_t i = 0; i < b; ++i)
        if (const int64_t* bad = bad_id(sp, ids_host + offs[i], offs[i + 1] - offs[i])) {
            set_err("%s: id %lld of list %lld is outside [0, %lld)", who, (long long)*bad, (long long)i, (long long)sp->n);
            return AS_EINVAL;
        }
    return AS_OK;
}
// the lists as 32-bit ids (item ids fit: space_new refuses n >= 2^31); dedupe: every list without its repeated ids, the first
// occurrence kept (offs: the new offsets) -- one pass with a stamp per item, the list that saw it last.  Does not depend on
// lambda_q: lists_call runs it on a helper thread beside the lambda_q step (no set_err here: the message is the caller's).
// false: out of host memory
static bool lists_ids32(const as_space* sp, const int64_t* ids_host, const int64_t* offs_in, int64_t b, bool dedupe, std::vector<int32_t>& ids,
                        std::vector<int64_t>& offs) {
    try {
        ids.resize((size_t)offs_in[b]);
        offs.assign(offs_in, offs_in + b + 1);
        if (!dedupe) {
            for (int64_t e = 0; e < offs_in[b]; ++e) ids[e] = (int32_t)ids_host[e];
            return true;
        }
        std::vector<int32_t> seen((size_t)sp->n, -1);
        int64_t o = 0;
        for (int64_t i = 0; i < b; ++i) {
            offs[i] = o;
            for (int64_t e = offs_in[i]; e < offs_in[i + 1]; ++e) {
                const int64_t j = ids_host[e];
                if (seen[j] == (int32_t)i) continue;
                seen[j] = (int32_t)i;
                ids[o++] = (int32_t)j;
            }
        }
        offs[b] = o;
    } catch (const std::bad_alloc&) {
        return false;
    }
    return true;
}
static int64_t host_ns_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}
// The four forms.  select: the first kk of every list, else every score.  sweep: the _taus forms (section 5.13) -- every tau finite,
// ONE lambda_q step with taus[0], the distinct taus through lists_run_taus, repeated taus copied here, counted in lsweep_count; the
// one-tau forms run lists_run and are counted in lists_count.  Either array: [0] calls, the driver's work counts (2, the sweeps
// 3), the lambda_q steps, then the host time the call spends serially: the checks, the wait for the helper thread after the
// lambda_q step, the work tables.
static as_status lists_call(const char* who, const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d,
                            const double* taus, int64_t ntau, bool sweep, const int64_t* ids_host, const int64_t* offs_host, bool select,
                            int64_t* out_idx, double* out_score, int64_t* out_len, double* out_scores, double* out_lambda_q,
                            int32_t* out_status) {
    std::atomic<int64_t>* count = sweep ? sp->lsweep_count : sp->lists_count;
    const int nwork = sweep ? 3 : 2;
    std::atomic<int64_t>& host_ns = count[nwork + 2];
    AS_TRY(subset_checks(who, sp, gr, d, taus, ntau));
    auto t0 = std::chrono::steady_clock::now();
    AS_TRY(lists_checks(who, sp, ids_host, offs_host, b));
    host_ns.fetch_add(host_ns_since(t0), std::memory_order_relaxed);
    count[0].fetch_add(1, std::memory_order_relaxed);
    if (b == 0 || ntau == 0) return AS_OK;
    std::vector<int32_t> ids;
    std::vector<int64_t> offs;
    bool ids_ok = true;
    std::thread helper;
    try {
        helper = std::thread([&] { ids_ok = lists_ids32(sp, ids_host, offs_host, b, select, ids, offs); });
    } catch (const std::system_error&) {   // no thread to be had: in line
        ids_ok = lists_ids32(sp, ids_host, offs_host, b, select, ids, offs);
    }
    std::vector<double> lq;
    std::vector<int32_t> st;
    const as_status ls = batch_lambda_step(who, sp, gr, queries, b, d, taus[0], &count[nwork + 1], lq, st, out_lambda_q, out_status);
    t0 = std::chrono::steady_clock::now();
    if (helper.joinable()) helper.join();
    host_ns.fetch_add(host_ns_since(t0), std::memory_order_relaxed);
    if (ls != AS_OK) return ls;
    if (!ids_ok) {
        set_err("%s: out of host memory for %lld ids", who, (long long)offs_host[b]);
        return AS_ENOMEM;
    }
    const int64_t kk = select ? hits_bound(sp, gr, sp->n) : 0;
    const TauSet ts(taus, sweep ? ntau : 0);   // (the one-tau forms: empty, nothing allocated)
    int64_t counts[4] = {0, 0, 0, 0};
    as_status r;
    {
        std::lock_guard<std::mutex> lk(sp->lmu);
        r = hipSetDevice(sp->device) == hipSuccess ? AS_OK : AS_EHIP;
        if (r != AS_OK) set_err("%s: hipSetDevice failed", who);
        else if (!sweep)
            r = lists_run(sp, ids.data(), offs.data(), queries, b, lq.data(), st.data(), taus[0], kk, out_idx, out_score, out_len, out_scores, counts);
        else
            r = lists_run_taus(sp, ids.data(), offs.data(), queries, b, lq.data(), st.data(), ts.uniq.data(), ts.size(), ts.row.data(), ntau, kk,
                               out_idx, out_score, out_len, out_scores, counts);
    }
    for (int c = 0; c < nwork; ++c) count[1 + c].fetch_add(counts[c], std::memory_order_relaxed);
    host_ns.fetch_add(counts[nwork], std::memory_order_relaxed);
    if (r != AS_OK || !sweep) return r;
    if (select) copy_repeated_lists(ts, b, kk, st.data(), out_idx, out_score, out_len);
    else copy_repeated_rows(ts, b, 0, offs_host, st.data(), out_scores);
    return AS_OK;
}

as_status as_score_lists_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                               const int64_t* ids_host, const int64_t* offsets_host, double* out_scores, double* out_lambda_q,
                               int32_t* out_status) {
    if (!sp || !gr || b < 0 || !offsets_host || (b > 0 && !queries) || (offsets_host[b] > 0 && (!ids_host || !out_scores))) {
        set_err("as_score_lists_batch: null argument");
        return AS_EINVAL;
    }
    return lists_call("as_score_lists_batch", sp, gr, queries, b, d, &tau, 1, false, ids_host, offsets_host, false, nullptr, nullptr, nullptr,
                      out_scores, out_lambda_q, out_status);
}

as_status as_search_lists_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                const int64_t* ids_host, const int64_t* offsets_host, int64_t* out_idx, double* out_score, int64_t* out_len,
                                double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || b < 0 || !offsets_host || (b > 0 && (!queries || !out_len)) || (offsets_host[b] > 0 && (!ids_host || !out_idx || !out_score))) {
        set_err("as_search_lists_batch: null argument");
        return AS_EINVAL;
    }
    return lists_call("as_search_lists_batch", sp, gr, queries, b, d, &tau, 1, false, ids_host, offsets_host, true, out_idx, out_score, out_len,
                      nullptr, out_lambda_q, out_status);
}

as_status as_lists_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_lists_counters", sp, out, n, sp ? sp->lists_count : nullptr, 5);
}

double as_lists_kernel_us(const as_space* sp) {
    if (!sp) return 0.0;
    std::lock_guard<std::mutex> lk(sp->lmu);
    return lists_kernel_us(sp->lists_ws);
}

// ---------------------------------------------------------------- tau sweeps over a subset (extension)
// The candidates of one sweep; the launches and tau planes the driver wrote into `counts` are counted when it goes.  It lives in
// a block of its own: the lock is released before the caller copies the repeated taus.
namespace {
struct SweepCandidates : Candidates {
    using Candidates::Candidates;
    int64_t counts[2] = {0, 0};
    ~SweepCandidates() {
        sp->ssweep_count[1].fetch_add(counts[0], std::memory_order_relaxed);
        sp->ssweep_count[2].fetch_add(counts[1], std::memory_order_relaxed);
    }
};
}  // namespace

as_status as_search_subset_taus(const as_space* sp, const as_graph* gr, const double* query, int64_t d, const double* taus, int64_t ntau,
                                const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q) {
    if (!sp || !gr || !query || !sub || ntau < 0 || (ntau > 0 && (!taus || !out_len || (sub->m > 0 && (!out_idx || !out_score))))) {
        set_err("as_search_subset_taus: null argument");
        return AS_EINVAL;
    }
    for (int64_t j = 0; j < ntau; ++j) out_len[j] = 0;
    AS_TRY(own_subset("as_search_subset_taus", sp, sub));
    AS_TRY(subset_checks("as_search_subset_taus", sp, gr, d, taus, ntau));
    if (ntau == 0) return AS_OK;
    sp->ssweep_count[0].fetch_add(1, std::memory_order_relaxed);
    double lq = 0.0;
    AS_TRY(lambda_step(sp, gr, query, d, taus[0], &sp->ssweep_count[3], &lq, out_lambda_q));
    if (sub->m == 0) return AS_OK;
    const int64_t kk = hits_bound(sp, gr, sub->m);
    const TauSet ts(taus, ntau);
    {
        SweepCandidates c("as_search_subset_taus", sp, sub);
        AS_TRY(c.status);
        AS_TRY(c.fail(subset_sweep_run(sp, c.w, c.m, query, lq, ts.uniq.data(), ts.size(), ts.row.data(), kk, out_idx, out_score, out_len,
                                       nullptr, c.counts)));
    }
    copy_repeated_lists(ts, 1, kk, nullptr, out_idx, out_score, out_len);
    return AS_OK;
}

as_status as_score_items_taus(const as_space* sp, const as_graph* gr, const double* query, int64_t d, const double* taus, int64_t ntau,
                              const int64_t* ids_host, int64_t m, double* out_scores, double* out_lambda_q) {
    if (!sp || !gr || !query || ntau < 0 || m < 0 || (ntau > 0 && !taus) || (m > 0 && !ids_host) || (ntau > 0 && m > 0 && !out_scores)) {
        set_err("as_score_items_taus: null argument");
        return AS_EINVAL;
    }
    AS_TRY(ids_in_range("as_score_items_taus", sp, ids_host, m));
    AS_TRY(subset_checks("as_score_items_taus", sp, gr, d, taus, ntau));
    if (ntau == 0) return AS_OK;
    sp->ssweep_count[0].fetch_add(1, std::memory_order_relaxed);
    double lq = 0.0;
    AS_TRY(lambda_step(sp, gr, query, d, taus[0], &sp->ssweep_count[3], &lq, out_lambda_q));
    if (m == 0) return AS_OK;
    std::vector<int32_t> ids;
    AS_TRY(checked_ids("as_score_items_taus", ids_host, m, ids));
    const TauSet ts(taus, ntau);
    {
        SweepCandidates c("as_score_items_taus", sp, ids.data(), m);
        AS_TRY(c.status);
        AS_TRY(c.fail(subset_sweep_run(sp, c.w, m, query, lq, ts.uniq.data(), ts.size(), ts.row.data(), 0, nullptr, nullptr, nullptr, out_scores,
                                       c.counts)));
    }
    copy_repeated_rows(ts, 1, m, nullptr, nullptr, out_scores);
    return AS_OK;
}

as_status as_search_subset_batch_taus(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, const double* taus,
                                      int64_t ntau, const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len,
                                      double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || !sub || b < 0 || ntau < 0 || (b > 0 && !queries) || (ntau > 0 && !taus) ||
        (b > 0 && ntau > 0 && (!out_len || (sub->m > 0 && (!out_idx || !out_score))))) {
        set_err("as_search_subset_batch_taus: null argument");
        return AS_EINVAL;
    }
    for (int64_t p = 0; p < b * ntau; ++p) out_len[p] = 0;
    AS_TRY(own_subset("as_search_subset_batch_taus", sp, sub));
    AS_TRY(subset_checks("as_search_subset_batch_taus", sp, gr, d, taus, ntau));
    if (b == 0 || ntau == 0) return AS_OK;
    sp->ssweep_count[0].fetch_add(1, std::memory_order_relaxed);
    std::vector<double> lq;
    std::vector<int32_t> st;
    AS_TRY(batch_lambda_step("as_search_subset_batch_taus", sp, gr, queries, b, d, taus[0], &sp->ssweep_count[3], lq, st, out_lambda_q, out_status));
    if (sub->m == 0) return AS_OK;
    const int64_t kk = hits_bound(sp, gr, sub->m);
    const TauSet ts(taus, ntau);
    {
        SweepCandidates c("as_search_subset_batch_taus", sp, sub);
        AS_TRY(c.status);
        AS_TRY(c.fail(subset_batch_sweep_run(sp, c.w, c.m, queries, b, lq.data(), st.data(), ts.uniq.data(), ts.size(), ts.row.data(), ntau, kk,
                                             out_idx, out_score, out_len, nullptr, c.counts)));
    }
    copy_repeated_lists(ts, b, kk, nullptr, out_idx, out_score, out_len);
    return AS_OK;
}

as_status as_score_items_batch_taus(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, const double* taus,
                                    int64_t ntau, const int64_t* ids_host, int64_t m, double* out_scores, double* out_lambda_q,
                                    int32_t* out_status) {
    if (!sp || !gr || b < 0 || ntau < 0 || m < 0 || (b > 0 && !queries) || (ntau > 0 && !taus) || (m > 0 && !ids_host) ||
        (b > 0 && ntau > 0 && m > 0 && !out_scores)) {
        set_err("as_score_items_batch_taus: null argument");
        return AS_EINVAL;
    }
    AS_TRY(ids_in_range("as_score_items_batch_taus", sp, ids_host, m));
    AS_TRY(subset_checks("as_score_items_batch_taus", sp, gr, d, taus, ntau));
    if (b == 0 || ntau == 0) return AS_OK;
    sp->ssweep_count[0].fetch_add(1, std::memory_order_relaxed);
    std::vector<double> lq;
    std::vector<int32_t> st;
    AS_TRY(batch_lambda_step("as_score_items_batch_taus", sp, gr, queries, b, d, taus[0], &sp->ssweep_count[3], lq, st, out_lambda_q, out_status));
    if (m == 0) return AS_OK;
    std::vector<int32_t> ids;
    AS_TRY(checked_ids("as_score_items_batch_taus", ids_host, m, ids));
    const TauSet ts(taus, ntau);
    {
        SweepCandidates c("as_score_items_batch_taus", sp, ids.data(), m);
        AS_TRY(c.status);
        AS_TRY(c.fail(subset_batch_sweep_run(sp, c.w, m, queries, b, lq.data(), st.data(), ts.uniq.data(), ts.size(), ts.row.data(), ntau, 0,
                                             nullptr, nullptr, nullptr, out_scores, c.counts)));
    }
    copy_repeated_rows(ts, b, m, nullptr, st.data(), out_scores);
    return AS_OK;
}

as_status as_subset_sweep_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_subset_sweep_counters", sp, out, n, sp ? sp->ssweep_count : nullptr, 4);
}

// ---------------------------------------------------------------- tau sweeps over per-query lists (extension)
as_status as_score_lists_batch_taus(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, const double* taus,
                                    int64_t ntau, const int64_t* ids_host, const int64_t* offsets_host, double* out_scores,
                                    double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || b < 0 || ntau < 0 || !offsets_host || (b > 0 && !queries) || (ntau > 0 && !taus) ||
        (offsets_host[b] > 0 && (!ids_host || (ntau > 0 && !out_scores)))) {
        set_err("as_score_lists_batch_taus: null argument");
        return AS_EINVAL;
    }
    return lists_call("as_score_lists_batch_taus", sp, gr, queries, b, d, taus, ntau, true, ids_host, offsets_host, false, nullptr, nullptr,
                      nullptr, out_scores, out_lambda_q, out_status);
}

as_status as_search_lists_batch_taus(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, const double* taus,
                                     int64_t ntau, const int64_t* ids_host, const int64_t* offsets_host, int64_t* out_idx, double* out_score,
                                     int64_t* out_len, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || b < 0 || ntau < 0 || !offsets_host || (b > 0 && !queries) || (ntau > 0 && !taus) || (b > 0 && ntau > 0 && !out_len) ||
        (offsets_host[b] > 0 && (!ids_host || (ntau > 0 && (!out_idx || !out_score))))) {
        set_err("as_search_lists_batch_taus: null argument");
        return AS_EINVAL;
    }
    return lists_call("as_search_lists_batch_taus", sp, gr, queries, b, d, taus, ntau, true, ids_host, offsets_host, true, out_idx, out_score,
                      out_len, nullptr, out_lambda_q, out_status);
}

as_status as_lists_sweep_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_lists_sweep_counters", sp, out, n, sp ? sp->lsweep_count : nullptr, 6);
}

// One batched tau sweep over b > 1 queries for nt <= TAU_GROUP distinct taus in [0, 1] (under sp->bmu): as_search_batch's
// workspaces, passes, pairs and pipelining, the scorer tail once per (query, tau) pair.  Pair (i, j): pidx / psc +
// (i * nt + j) * topk, plen / pst [i * nt + j], plq [i]; pst -1: left to the single search.  *passes: passes that ran the tail.
static as_status batch_sweep_run(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, const double* gt,
                                 int nt, int64_t topk, int64_t* pidx, double* psc, int64_t* plen, double* plq, int32_t* pst,
                                 int64_t* passes) {
    int unit = 1;
    AS_TRY(batch_workspaces(sp, gr, b, &unit));
    return batch_passes(
        sp, unit, b,
        [&](as_query* w0, int64_t i0, int nb0, as_query* w1, int64_t i1, int nb1) {
            return w1 ? search_batch_sweep_launch_pair(w0, w1, queries + i0 * d, nb0, queries + i1 * d, nb1, d, gt, nt)
                      : search_batch_sweep_launch(w0, queries + i0 * d, nb0, d, gt, nt);
        },
        [&](as_query* w, int64_t i0, int nb) -> as_status {
            AS_TRY(search_batch_sweep_collect(w, nb, gt, nt, topk, pidx + i0 * nt * topk, psc + i0 * nt * topk, plen + i0 * nt, plq + i0, pst + i0 * nt));
            *passes += query_sweep_ran(w);
            return AS_OK;
        });
}

// Extension: b queries under ntau taus -- entry (i, j) is what as_search returns for query i and taus[j].  Equal taus are
// computed once.  Where as_search_batch batches (b > 1, no force_exact or search_mode, no feature lambdas) the distinct taus in
// [0, 1] share batched passes, up to TAU_GROUP per pass (batch_sweep_run); every other tau takes as_search_batch's own route,
// and every pair a shared pass does not serve is redone by the single search with its own tau.
as_status as_search_batch_taus(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, const double* taus,
                               int64_t ntau, int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status) {
    if (!sp || !gr || b < 0 || ntau < 0 || (b > 0 && !queries) || (b > 0 && ntau > 0 && (!taus || !out_idx || !out_score || !out_len))) {
        set_err("as_search_batch_taus: null argument");
        return AS_EINVAL;
    }
    if (d != sp->d) {
        set_err("query length %lld must match nfeatures %lld", (long long)d, (long long)sp->d);
        return AS_EINVAL;
    }
    AS_TRY(graph_matches(sp, gr, "as_search_batch_taus"));
    if (b == 0 || ntau == 0) return AS_OK;
    sp->bsweep_count[0].fetch_add(1, std::memory_order_relaxed);
    const int64_t topk = std::min<int64_t>(gr->gp.topk, sp->n);
    // distinct taus (bit patterns), in order of first appearance
    std::vector<double> uniq;
    std::vector<int64_t> slot((size_t)ntau);
    for (int64_t j = 0; j < ntau; ++j) {
        int64_t u = 0;
        while (u < (int64_t)uniq.size() && memcmp(&uniq[u], &taus[j], sizeof(double)) != 0) ++u;
        if (u == (int64_t)uniq.size()) uniq.push_back(taus[j]);
        slot[j] = u;
    }
    const int64_t nu = (int64_t)uniq.size();
    const bool batched = !sp->opts.force_exact && (sp->opts.search_mode & 3) == 0 && b > 1 && gr->lambda_mode != AS_LAMBDA_FEATURE;
    std::vector<int64_t> shared;
    std::vector<char> is_shared((size_t)nu, 0);
    for (int64_t u = 0; u < nu && batched; ++u)
        if (uniq[u] >= 0.0 && uniq[u] <= 1.0) {
            shared.push_back(u);
            is_shared[u] = 1;
        }
    // per distinct tau: [b][topk] lists, [b] lengths and statuses
    const size_t per = (size_t)(b * std::max<int64_t>(topk, 1));
    std::vector<int64_t> uidx(per * nu), ulen((size_t)(b * nu), 0);
    std::vector<double> usc(per * nu), lq((size_t)b, 0.0);
    std::vector<int32_t> ust((size_t)(b * nu), 0);
    int64_t passes = 0, served = 0, redone = 0;
    if (!shared.empty()) {
        std::lock_guard<std::mutex> lock(sp->bmu);
        AS_HIP(hipSetDevice(sp->device));
        for (size_t g0 = 0; g0 < shared.size(); g0 += TAU_GROUP) {
            const int nt = (int)std::min<size_t>(TAU_GROUP, shared.size() - g0);
            double gt[TAU_GROUP];
            for (int j = 0; j < nt; ++j) gt[j] = uniq[shared[g0 + j]];
            std::vector<int64_t> pidx((size_t)(b * nt * std::max<int64_t>(topk, 1))), plen((size_t)(b * nt), 0);
            std::vector<double> psc(pidx.size());
            std::vector<int32_t> pst((size_t)(b * nt), -1);
            AS_TRY(batch_sweep_run(sp, gr, queries, b, d, gt, nt, topk, pidx.data(), psc.data(), plen.data(), lq.data(), pst.data(), &passes));
            for (int64_t i = 0; i < b; ++i)
                for (int j = 0; j < nt; ++j) {
                    const int64_t u = shared[g0 + j], p = i * nt + j;
                    ust[u * b + i] = pst[p];
                    if (pst[p] == -1) continue;
                    served += 1;
                    ulen[u * b + i] = plen[p];
                    for (int64_t t = 0; t < plen[p]; ++t) {
                        uidx[u * per + i * topk + t] = pidx[p * topk + t];
                        usc[u * per + i * topk + t] = psc[p * topk + t];
                    }
                }
        }
    }
    sp->bsweep_count[1].fetch_add(passes, std::memory_order_relaxed);
    sp->bsweep_count[2].fetch_add(served, std::memory_order_relaxed);
    // the other taus: as_search_batch's route for each
    for (int64_t u = 0; u < nu; ++u) {
        if (is_shared[u]) continue;
        AS_TRY(as_search_batch(sp, gr, queries, b, d, uniq[u], uidx.data() + u * per, usc.data() + u * per, ulen.data() + u * b, lq.data(),
                               ust.data() + u * b));
    }
    // the pairs a shared pass left: the single search with their own tau
    for (int64_t u = 0; u < nu; ++u) {
        if (!is_shared[u]) continue;
        for (int64_t i = 0; i < b; ++i) {
            if (ust[u * b + i] != -1) continue;
            redone += 1;
            double l = 0.0;
            const as_status s1 = search_pooled(sp, gr, queries + i * d, d, uniq[u], uidx.data() + u * per + i * topk, usc.data() + u * per + i * topk,
                                               ulen.data() + u * b + i, &l);
            lq[i] = l;
            ust[u * b + i] = (int32_t)s1;
            if (s1 != AS_OK && s1 != AS_EZEROLAMBDA) {
                sp->bsweep_count[3].fetch_add(redone, std::memory_order_relaxed);
                return s1;
            }
        }
    }
    sp->bsweep_count[3].fetch_add(redone, std::memory_order_relaxed);
    for (int64_t i = 0; i < b; ++i) {
        int32_t st = AS_OK;
        for (int64_t j = 0; j < ntau; ++j) {
            const int64_t u = slot[j];
            const int32_t su = ust[u * b + i];
            const int64_t len = su == AS_EZEROLAMBDA ? 0 : ulen[u * b + i];
            if (su == AS_EZEROLAMBDA) st = AS_EZEROLAMBDA;
            for (int64_t t = 0; t < len; ++t) {
                out_idx[(i * ntau + j) * topk + t] = uidx[u * per + i * topk + t];
                out_score[(i * ntau + j) * topk + t] = usc[u * per + i * topk + t];
            }
            out_len[i * ntau + j] = len;
        }
        if (out_lambda_q) out_lambda_q[i] = lq[i];
        if (out_status) out_status[i] = st;
    }
    return AS_OK;
}

as_status as_batch_sweep_counters(const as_space* sp, int64_t* out, int32_t n) {
    return counters_out("as_batch_sweep_counters", sp, out, n, sp ? sp->bsweep_count : nullptr, 4);
}

// ---------------------------------------------------------------- accessors
int64_t as_nitems(const as_space* sp) { return sp ? sp->n : 0; }
int64_t as_nfeatures(const as_space* sp) { return sp ? sp->d : 0; }
int64_t as_nnodes(const as_graph* gr) { return gr ? gr->n : 0; }
int64_t as_graph_nnz(const as_graph* gr) { return gr ? gr->nnz + gr->n : 0; }
double as_graph_tau0(const as_graph* gr) { return gr ? gr->tau0 : 0.0; }
int32_t as_graph_lambda_mode(const as_graph* gr) { return gr ? gr->lambda_mode : 0; }
const double* as_lambdas_dev(const as_space* sp) { return sp ? sp->lam64 : nullptr; }

as_status as_get_item(const as_space* sp, int64_t idx, double* out_vec, double* out_lambda) {
    if (!sp || !out_vec) {
        set_err("as_get_item: null argument");
        return AS_EINVAL;
    }
    if (idx < 0 || idx >= sp->n) {  // src/lib.rs:101-107
        set_err("index %lld out of range [0, %lld)", (long long)idx, (long long)sp->n);
        return AS_EINVAL;
    }
    AS_HIP(hipSetDevice(sp->device));
    if (sp->x64) {
        AS_HIP(hipMemcpy(out_vec, sp->x64 + idx * sp->d, sizeof(double) * sp->d, hipMemcpyDeviceToHost));
    } else {
        std::vector<float> tmp(sp->d);
        AS_HIP(hipMemcpy(tmp.data(), sp->x32 + idx * sp->dp, sizeof(float) * sp->d, hipMemcpyDeviceToHost));
        for (int64_t c = 0; c < sp->d; ++c) out_vec[c] = (double)tmp[c];
    }
    if (out_lambda) AS_HIP(hipMemcpy(out_lambda, sp->lam64 + idx, sizeof(double), hipMemcpyDeviceToHost));
    return AS_OK;
}

as_status as_lambdas(const as_space* sp, double* out) {
    if (!sp || !out) {
        set_err("as_lambdas: null argument");
        return AS_EINVAL;
    }
    AS_HIP(hipSetDevice(sp->device));
    AS_HIP(hipMemcpy(out, sp->lam64, sizeof(double) * sp->n, hipMemcpyDeviceToHost));
    return AS_OK;
}

as_status as_get_graph_params(const as_graph* gr, as_graph_params* out) {
    if (!gr || !out) {
        set_err("as_get_graph_params: null argument");
        return AS_EINVAL;
    }
    *out = gr->gp;
    return AS_OK;
}

as_status as_graph_degrees(const as_graph* gr, double* out) {
    if (!gr || !out) {
        set_err("as_graph_degrees: null argument");
        return AS_EINVAL;
    }
    AS_HIP(hipSetDevice(gr->device));
    AS_HIP(hipMemcpy(out, gr->deg, sizeof(double) * gr->n, hipMemcpyDeviceToHost));
    return AS_OK;
}

as_status as_graph_csr(const as_graph* gr, int64_t* indptr, int64_t* indices, double* values) {
    if (!gr || !indptr || !indices || !values) {
        set_err("as_graph_csr: null argument");
        return AS_EINVAL;
    }
    AS_HIP(hipSetDevice(gr->device));
    const int64_t n = gr->n, nnz = gr->nnz;
    std::vector<int64_t> ip(n + 1);
    std::vector<int32_t> col(std::max<int64_t>(nnz, 1));
    std::vector<double> lap(std::max<int64_t>(nnz, 1)), deg(n);
    AS_HIP(hipMemcpy(ip.data(), gr->indptr, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost));
    if (nnz) {
        AS_HIP(hipMemcpy(col.data(), gr->indices, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost));
        AS_HIP(hipMemcpy(lap.data(), gr->lap, sizeof(double) * nnz, hipMemcpyDeviceToHost));
    }
    AS_HIP(hipMemcpy(deg.data(), gr->deg, sizeof(double) * n, hipMemcpyDeviceToHost));
    // insert the diagonal keeping columns ascending: normalised Laplacian 1 for connected nodes, 0 for isolated
    // ones; feature graph (L = D - W) the degree
    const bool comb = gr->lambda_mode == AS_LAMBDA_FEATURE;
    int64_t w = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t i = r + gr->row0;   // a sharded graph holds the rows [row0, row0 + n): the diagonal sits at column row0 + r
        indptr[r] = w;
        bool placed = false;
        for (int64_t e = ip[r]; e < ip[r + 1]; ++e) {
            if (!placed && col[e] > i) {
                indices[w] = i;
                values[w++] = comb ? deg[r] : (deg[r] > 0.0 ? 1.0 : 0.0);
                placed = true;
            }
            indices[w] = col[e];
            values[w++] = lap[e];
        }
        if (!placed) {
            indices[w] = i;
            values[w++] = comb ? deg[r] : (deg[r] > 0.0 ? 1.0 : 0.0);
        }
    }
    indptr[n] = w;
    return AS_OK;
}

as_status as_graph_csr_dist(const as_graph* gr, int64_t* indptr, int64_t* indices, double* dist) {
    if (!gr || !indptr || (gr->nnz > 0 && (!indices || !dist))) {
        set_err("as_graph_csr_dist: null argument");
        return AS_EINVAL;
    }
    if (gr->lambda_mode == AS_LAMBDA_FEATURE || (gr->nnz > 0 && !gr->dist)) {
        set_err("as_graph_csr_dist: a feature-mode graph stores no distances");
        return AS_EUNSUPPORTED;
    }
    AS_HIP(hipSetDevice(gr->device));
    const int64_t n = gr->n, nnz = gr->nnz;
    AS_HIP(hipMemcpy(indptr, gr->indptr, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost));
    if (nnz) {
        std::vector<int32_t> col(nnz);
        AS_HIP(hipMemcpy(col.data(), gr->indices, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost));
        AS_HIP(hipMemcpy(dist, gr->dist, sizeof(double) * nnz, hipMemcpyDeviceToHost));
        std::copy(col.begin(), col.end(), indices);
    }
    return AS_OK;
}

as_status as_last_search_stats(const as_space* sp, double* out, int32_t n) {
    if (!sp || !out || !sp->qcache) {
        set_err("as_last_search_stats: no search has run on this space");
        return AS_EINVAL;
    }
    return as_query_stats(sp->qcache, out, n);
}

as_status as_search_counters(const as_space* sp, int64_t* out, int32_t n) {
    if (!sp || !out) {
        set_err("as_search_counters: null argument");
        return AS_EINVAL;
    }
    std::lock_guard<std::mutex> lk(sp->qmu);
    for (int i = 0; i < n && i < 6; ++i) out[i] = sp->scount[i];
    for (int i = 6; i < n && i < 8; ++i) out[i] = sp->nib_count[i - 6].load(std::memory_order_relaxed);
    return AS_OK;
}

as_status as_build_stats(const as_graph* gr, double* out, int32_t n) {
    if (!gr || !out) {
        set_err("as_build_stats: null argument");
        return AS_EINVAL;
    }
    for (int i = 0; i < n && i < 10; ++i) out[i] = gr->stats[i];
    return AS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- index persistence
// One flat little-endian file: header, the items (fp64 when an fp64 copy is kept, else the exact
// fp32 values), lambdas, and the graph arrays.  Loading re-ingests the items (norms and the padded
// fp32 layout are recomputed deterministically) and uploads the rest; no k-NN work is redone.
// The header carries its own size and a format version; the loader checks the file length against the
// header-derived sizes before allocating anything and validates the CSR it is about to trust.
namespace {
struct IndexHeader {
    char magic[8];           // "ASIDX04\0"
    int32_t header_bytes;    // sizeof(IndexHeader) of the writer
    int32_t version;         // 4
    int64_t n, d, nnz;       // items held by this file, features, adjacency entries
    int64_t nnodes;          // graph rows in this file: the items of the whole index (item mode, replicated graph), this
                             // shard's n rows (item mode, sharded graph: graph_ncols > 0) or d (feature mode)
    int64_t graph_ncols;     // sharded item graph: the items its columns range over; 0 for a whole graph.  Feature mode: the
                             // items the lambdas were ranked over (all ranks' rows)
    int64_t graph_row0;      // sharded item graph: its first row (== row_offset)
    int64_t row_offset;      // global index of this file's first item (0 for a whole index)
    int32_t has_f64, metric, kernel, lambda_mode;
    as_graph_params gp;
    double tau0;
};
constexpr int32_t INDEX_VERSION = 4;

template <typename T>
as_status dev_to_file(FILE* f, const T* dev, size_t count) {
    std::vector<T> h(std::max<size_t>(count, 1));
    if (count) AS_HIP(hipMemcpy(h.data(), dev, sizeof(T) * count, hipMemcpyDeviceToHost));
    if (count && fwrite(h.data(), sizeof(T), count, f) != count) {
        set_err("as_index_save: short write");
        return AS_EINVAL;
    }
    return AS_OK;
}
template <typename T>
as_status file_to_host(FILE* f, std::vector<T>& h, size_t count) {
    h.resize(std::max<size_t>(count, 1));
    if (count && fread(h.data(), sizeof(T), count, f) != count) {
        set_err("as_index_load: truncated file");
        return AS_EINVAL;
    }
    return AS_OK;
}
template <typename T>
as_status host_to_dev(const std::vector<T>& h, T** dev, size_t count) {
    AS_HIP(hipMalloc(dev, sizeof(T) * std::max<size_t>(count, 1)));
    if (count) AS_HIP(hipMemcpy(*dev, h.data(), sizeof(T) * count, hipMemcpyHostToDevice));
    return AS_OK;
}
template <typename T>
as_status file_to_dev(FILE* f, T** dev, size_t count) {
    std::vector<T> h;
    AS_TRY(file_to_host(f, h, count));
    return host_to_dev(h, dev, count);
}
// bytes the arrays behind the header occupy, or -1 when the header's sizes are not credible
int64_t payload_bytes(const IndexHeader& h) {
    const int64_t lim = (int64_t)1 << 46;
    if (h.n <= 0 || h.d <= 0 || h.nnz < 0 || h.nnodes <= 0 || h.n >= ((int64_t)1 << 31) || h.d >= ((int64_t)1 << 31) ||
        h.nnz > lim || h.n > lim / h.d)
        return -1;
    const int64_t item = h.has_f64 ? 8 : 4;
    int64_t b = h.n * h.d * item + h.n * 8;                 // items, lambdas
    b += (h.nnodes + 1) * 8 + h.nnz * 4 + h.nnz * 8 * 4;    // indptr, indices, dist gy w lap
    b += h.nnodes * 8;                                      // deg
    if (h.lambda_mode == AS_LAMBDA_FEATURE) b += h.n * 8 * 2 + h.d * 8;   // E, G, colm
    else b += h.nnodes * 8 * 3;                             // ny, E, G of every graph node
    return b;
}
}  // namespace

extern "C" {

as_status as_index_save(const as_space* sp, const as_graph* gr, const char* path) {
    if (!sp || !gr || !path) {
        set_err("as_index_save: null argument");
        return AS_EINVAL;
    }
    AS_HIP(hipSetDevice(sp->device));
    FILE* f = fopen(path, "wb");
    if (!f) {
        set_err("as_index_save: cannot open %s", path);
        return AS_EINVAL;
    }
    IndexHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, "ASIDX04", 8);
    h.header_bytes = (int32_t)sizeof(IndexHeader);
    h.version = INDEX_VERSION;
    h.n = sp->n; h.d = sp->d; h.nnz = gr->nnz; h.nnodes = gr->n; h.row_offset = sp->row_offset;
    h.graph_ncols = gr->lambda_mode == AS_LAMBDA_FEATURE ? gr->nitems : gr->ncols;   // feature mode: the items the lambdas were ranked over
    h.graph_row0 = gr->row0;
    h.has_f64 = sp->x64 ? 1 : 0; h.metric = gr->metric; h.kernel = gr->kernel; h.lambda_mode = gr->lambda_mode;
    h.gp = gr->gp; h.tau0 = gr->tau0;
    as_status s = fwrite(&h, sizeof(h), 1, f) == 1 ? AS_OK : AS_EINVAL;
    const size_t n = (size_t)sp->n, d = (size_t)sp->d, nnz = (size_t)gr->nnz, nn = (size_t)gr->n;
    if (s == AS_OK) {
        if (sp->x64) {
            s = dev_to_file(f, sp->x64, n * d);
        } else {
            std::vector<float> all(n * d);
            hipError_t e = hipMemcpy2D(all.data(), sizeof(float) * d, sp->x32, sizeof(float) * sp->dp, sizeof(float) * d, n, hipMemcpyDeviceToHost);
            if (e != hipSuccess) s = AS_EHIP;
            if (s == AS_OK && fwrite(all.data(), sizeof(float), n * d, f) != n * d) s = AS_EINVAL;
        }
    }
    if (s == AS_OK) s = dev_to_file(f, sp->lam64, n);
    if (s == AS_OK) s = dev_to_file(f, gr->indptr, nn + 1);
    if (s == AS_OK) s = dev_to_file(f, gr->indices, nnz);
    if (s == AS_OK) s = dev_to_file(f, gr->dist, nnz);
    if (s == AS_OK) s = dev_to_file(f, gr->gy, nnz);
    if (s == AS_OK) s = dev_to_file(f, gr->w, nnz);
    if (s == AS_OK) s = dev_to_file(f, gr->lap, nnz);
    if (s == AS_OK) s = dev_to_file(f, gr->deg, nn);
    if (gr->lambda_mode == AS_LAMBDA_FEATURE) {
        // a shard of a row-sharded index holds the energies of every item right after its build (e_rows == nitems) and
        // its own rows' after a load (e_rows == n): this file keeps its own rows' either way
        const int64_t eoff = gr->e_rows > sp->n ? sp->row_offset : 0;
        if (s == AS_OK && gr->e_rows < eoff + sp->n) {
            set_err("as_index_save: the graph holds %lld energies, the space rows [%lld, %lld)", (long long)gr->e_rows, (long long)eoff, (long long)(eoff + sp->n));
            s = AS_EINVAL;
        }
        if (s == AS_OK) s = dev_to_file(f, gr->E + eoff, n);
        if (s == AS_OK) s = dev_to_file(f, gr->G + eoff, n);
        if (s == AS_OK) s = dev_to_file(f, gr->colm, d);
    } else {
        if (s == AS_OK) s = dev_to_file(f, gr->ny, nn);
        if (s == AS_OK) s = dev_to_file(f, gr->E, nn);
        if (s == AS_OK) s = dev_to_file(f, gr->G, nn);
    }
    if (fclose(f) != 0 && s == AS_OK) s = AS_EINVAL;
    if (s != AS_OK && err_slot().empty()) set_err("as_index_save: write to %s failed", path);
    return s;
}

__global__ void lam32_kernel(int64_t n, const double* __restrict__ lam64, float* __restrict__ lam32) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lam32[i] = (float)lam64[i];
}

static as_status index_load_impl(FILE* f, const char* path, const as_opts* opts, as_space** out_space, as_graph** out_graph) {
    IndexHeader h;
    if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, "ASIDX04", 8) != 0 || h.header_bytes != (int32_t)sizeof(IndexHeader) ||
        h.version != INDEX_VERSION) {
        set_err("as_index_load: %s is not an arrowspace index file of format %d", path, INDEX_VERSION);
        return AS_EINVAL;
    }
    const int64_t need = payload_bytes(h);
    const bool modes_ok = (h.metric == AS_METRIC_L2 || h.metric == AS_METRIC_COSINE) &&
                          (h.kernel == AS_KERNEL_GAUSSIAN || h.kernel == AS_KERNEL_RATIONAL) &&
                          (h.lambda_mode == AS_LAMBDA_ITEM || h.lambda_mode == AS_LAMBDA_FEATURE) &&
                          (h.lambda_mode == AS_LAMBDA_FEATURE ? (h.nnodes == h.d && h.row_offset >= 0)
                          : h.graph_ncols ? (h.row_offset >= 0 && h.graph_row0 == h.row_offset && h.nnodes == h.n &&
                                             h.graph_ncols >= h.row_offset + h.n && h.graph_ncols < ((int64_t)1 << 31))
                                          : (h.row_offset >= 0 && h.graph_row0 == 0 && h.nnodes >= h.row_offset + h.n));
    as_graph_params gpr;
    if (need < 0 || !modes_ok || resolve_params(&h.gp, &gpr) != AS_OK || !(h.tau0 >= 0.0) || !(h.tau0 <= 1.0)) {
        set_err("as_index_load: %s has an inconsistent header", path);
        return AS_EINVAL;
    }
    {   // the file must hold exactly the arrays the header announces
        const long pos = ftell(f);
        if (pos < 0 || fseek(f, 0, SEEK_END) != 0) {
            set_err("as_index_load: cannot seek in %s", path);
            return AS_EINVAL;
        }
        const long end = ftell(f);
        if (fseek(f, pos, SEEK_SET) != 0 || (int64_t)(end - pos) != need) {
            set_err("as_index_load: %s is truncated or has trailing bytes (%lld payload bytes, header implies %lld)", path,
                    (long long)(end - pos), (long long)need);
            return AS_EINVAL;
        }
    }
    as_opts o{};
    if (opts) o = *opts;
    o.metric = h.metric;
    o.kernel = h.kernel;
    o.lambda_mode = h.lambda_mode;
    o.keep_f64 = h.has_f64 ? AS_KEEP_F64_ALWAYS : AS_KEEP_F64_AUTO;
    int dev = 0;
    AS_TRY(pick_device(&o, &dev));
    o.device = dev;
    as_space* sp = nullptr;
    as_graph* gr = nullptr;
    void* items = nullptr;
    const size_t n = (size_t)h.n, d = (size_t)h.d, nnz = (size_t)h.nnz, nn = (size_t)h.nnodes;
    as_status s = AS_OK;
    do {
        if (h.has_f64) {
            double* p = nullptr;
            s = file_to_dev(f, &p, n * d);
            items = p;
        } else {
            float* p = nullptr;
            s = file_to_dev(f, &p, n * d);
            items = p;
        }
        if (s != AS_OK) break;
        s = as_space_create_dev(items, h.has_f64 ? AS_DTYPE_F64 : AS_DTYPE_F32, h.n, h.d, h.d, &o, &sp);
        if (s != AS_OK) break;
        hipFree(sp->lam64);
        sp->lam64 = nullptr;
        s = file_to_dev(f, &sp->lam64, n);
        if (s != AS_OK) break;
        hipLaunchKernelGGL(lam32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sp->stream, h.n, sp->lam64, sp->lam32);
        gr = new as_graph();
        gr->device = dev; gr->n = h.nnodes; gr->nitems = h.row_offset + h.n; gr->nnz = h.nnz; gr->gp = gpr; gr->metric = h.metric; gr->kernel = h.kernel;
        gr->lambda_mode = h.lambda_mode; gr->tau0 = h.tau0; gr->row0 = h.graph_row0;
        if (h.lambda_mode == AS_LAMBDA_FEATURE) gr->nitems = std::max<int64_t>(gr->nitems, h.graph_ncols);
        else gr->ncols = h.graph_ncols;
        {   // the CSR is walked on trust afterwards: monotone row pointers ending at nnz, columns inside the graph
            std::vector<int64_t> ip;
            std::vector<int32_t> col;
            if ((s = file_to_host(f, ip, nn + 1)) != AS_OK) break;
            if ((s = file_to_host(f, col, nnz)) != AS_OK) break;
            bool ok = ip[0] == 0 && ip[nn] == h.nnz;
            for (size_t i = 0; ok && i < nn; ++i) ok = ip[i] <= ip[i + 1];
            const int64_t colmax = h.lambda_mode != AS_LAMBDA_FEATURE && h.graph_ncols ? h.graph_ncols : h.nnodes;   // (feature mode: the field counts items)
            for (size_t e = 0; ok && e < nnz; ++e) ok = col[e] >= 0 && (int64_t)col[e] < colmax;
            if (!ok) {
                set_err("as_index_load: %s holds an inconsistent graph (row pointers or column indices out of range)", path);
                s = AS_EINVAL;
                break;
            }
            if ((s = host_to_dev(ip, &gr->indptr, nn + 1)) != AS_OK) break;
            if ((s = host_to_dev(col, &gr->indices, nnz)) != AS_OK) break;
        }
        if ((s = file_to_dev(f, &gr->dist, nnz)) != AS_OK) break;
        if ((s = file_to_dev(f, &gr->gy, nnz)) != AS_OK) break;
        if ((s = file_to_dev(f, &gr->w, nnz)) != AS_OK) break;
        if ((s = file_to_dev(f, &gr->lap, nnz)) != AS_OK) break;
        if ((s = file_to_dev(f, &gr->deg, nn)) != AS_OK) break;
        if (h.lambda_mode == AS_LAMBDA_FEATURE) {
            if ((s = file_to_dev(f, &gr->E, n)) != AS_OK) break;
            if ((s = file_to_dev(f, &gr->G, n)) != AS_OK) break;
            gr->e_rows = h.n;
            if ((s = file_to_dev(f, &gr->colm, d)) != AS_OK) break;
            if ((s = feat_edges_from_csr(gr, sp->stream)) != AS_OK) break;
            sp->row_offset = h.row_offset;
        } else {
            if ((s = file_to_dev(f, &gr->ny, nn)) != AS_OK) break;
            if ((s = file_to_dev(f, &gr->E, nn)) != AS_OK) break;
            if ((s = file_to_dev(f, &gr->G, nn)) != AS_OK) break;
            sp->row_offset = h.row_offset;
        }
        if (hipStreamSynchronize(sp->stream) != hipSuccess) s = AS_EHIP;
    } while (0);
    if (items) hipFree(items);
    if (s != AS_OK) {
        if (gr) as_free_graph(gr);
        if (sp) as_free_space(sp);
        return s;
    }
    *out_space = sp;
    *out_graph = gr;
    return AS_OK;
}

as_status as_index_load(const char* path, const as_opts* opts, as_space** out_space, as_graph** out_graph) {
    if (!path || !out_space || !out_graph) {
        set_err("as_index_load: null argument");
        return AS_EINVAL;
    }
    *out_space = nullptr;
    *out_graph = nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) {
        set_err("as_index_load: cannot open %s", path);
        return AS_EINVAL;
    }
    as_status s;
    try {
        s = index_load_impl(f, path, opts, out_space, out_graph);
    } catch (const std::bad_alloc&) {   // nothing may unwind through the C ABI
        set_err("as_index_load: out of host memory reading %s", path);
        s = AS_ENOMEM;
    }
    fclose(f);
    return s;
}

}  // extern "C"
