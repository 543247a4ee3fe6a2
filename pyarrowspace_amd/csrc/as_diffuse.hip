// Graph-diffusion search (section 5.22): f <- alpha S f + (1 - alpha) y over the item graph the index
// keeps on the device, S = -lap (the stored off-diagonal entries of D^-1/2 A D^-1/2), y the hit list of the ordinary route.
// f is [N][C] doubles, item-major, C = 1, 16 or 64 columns (queries) of a chunk, in two buffers used ping-pong.  A step is one
// launch of a step kernel, which writes fl(alpha acc) for every (row, column), and one launch of the seed kernel, which adds
// fl((1 - alpha) y) at the seeds' cells (y is kept sparse: a table of (item, column, value) per chunk; the (item, column) pairs
// of a chunk are distinct, so no atomics are needed).  Every product and every sum is rounded once -- plain operators under the
// contract-off pragma below (HIP's __dmul_rn / __dadd_rn are plain operators of a header compiled with contraction on, which
// the compiler fused) -- and a row's sum runs in CSR order: the result has the bits of the numpy reference, whatever the
// column chunk, the tile or the grid.
// Entry points: as_api.hip (as_search_diffuse, as_search_diffuse_batch, as_score_diffuse_batch, as_diffuse_seeds).
// The call frame, the seed table and the output paths are functions of their own (as_diffuse.hpp): the S20 solve
// (as_diffuse_solve.hip) runs on the same work buffers and ends in the same outputs.
#include <algorithm>
#include <atomic>
#include <new>
#include <vector>

#include "as_diffuse.hpp"

// S19 rounds every product and every sum once: no multiply of this file may be fused with the add behind it
#pragma clang fp contract(off)

namespace as {

struct DiffuseArgs {
    const int64_t* indptr;    // [n + 1]
    const int32_t* indices;   // [nnz]
    const double* lap;        // [nnz]: S_e = -lap[e]
    const double* fin;        // [n][C]
    double* fout;             // [n][C]: fl(alpha acc); the seed kernel adds fl((1 - alpha) y) behind
    int64_t n;
    double alpha;
    int tile;                 // the C = 1 kernel: edges per LDS tile
};

// C = 1, the CSR-stream shape.  A block owns groups of DIF_THREADS consecutive rows (grid-stride over the groups).  The edges of a
// group are one contiguous run of the CSR: the block streams it through LDS a tile at a time -- lap, indices and the gathered
// f[col] read coalesced, the product S_e f[col_e] formed on the way in -- and after each tile one lane per row adds the products
// of its row that lie in the tile, in CSR order, to the acc it keeps in a register: a row longer than the tile carries its acc
// across tiles in the same order.  Every edge is read once.
__global__ __launch_bounds__(DIF_THREADS) void diffuse_step1_kernel(DiffuseArgs a) {
    extern __shared__ double dif_prod[];
    const int tid = threadIdx.x, T = a.tile;
    const int64_t groups = (a.n + DIF_THREADS - 1) / DIF_THREADS;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t first = g * DIF_THREADS, last = first + DIF_THREADS < a.n ? first + DIF_THREADS : a.n;
        const int64_t row = first + tid;
        const bool live = row < last;
        const int64_t rs = live ? a.indptr[row] : 0, re = live ? a.indptr[row + 1] : 0;
        const int64_t e0 = a.indptr[first], e1 = a.indptr[last];
        double acc = 0.0;
        for (int64_t s0 = e0; s0 < e1; s0 += T) {
            const int64_t s1 = s0 + T < e1 ? s0 + T : e1;
            for (int64_t e = s0 + tid; e < s1; e += DIF_THREADS) dif_prod[e - s0] = -a.lap[e] * a.fin[a.indices[e]];
            __syncthreads();
            const int64_t lo = rs > s0 ? rs : s0, hi = re < s1 ? re : s1;
            for (int64_t e = lo; e < hi; ++e) acc = acc + dif_prod[e - s0];
            __syncthreads();   // the tile is read before the next one is written
        }
        if (live) a.fout[row] = a.alpha * acc;
    }
}

// C = CT > 1: lanes own columns.  A wave has 64 / CT rows in flight; the CT lanes of a row read S_e and col_e once (one address:
// a broadcast) and f[col_e][0 .. CT) as one contiguous segment, and each lane keeps the sequential chain of its (row, column).
// Grid-stride over the waves' row groups.  Four edges are loaded ahead of the chain.
template <int CT>
__global__ __launch_bounds__(DIF_THREADS) void diffuse_step_cols_kernel(DiffuseArgs a) {
    constexpr int RPW = 64 / CT;
    const int lane = threadIdx.x & 63, c = lane % CT, sub = lane / CT;
    const int64_t waves = (int64_t)gridDim.x * (DIF_THREADS / 64);
    for (int64_t r0 = ((int64_t)blockIdx.x * (DIF_THREADS / 64) + (threadIdx.x >> 6)) * RPW; r0 < a.n; r0 += waves * RPW) {
        const int64_t row = r0 + sub;
        if (row >= a.n) continue;
        const int64_t rs = a.indptr[row], re = a.indptr[row + 1];
        const double* __restrict__ f = a.fin + c;
        double acc = 0.0;
        int64_t e = rs;
        for (; e + 4 <= re; e += 4) {
            const double s0 = -a.lap[e], s1 = -a.lap[e + 1], s2 = -a.lap[e + 2], s3 = -a.lap[e + 3];
            const double v0 = f[(int64_t)a.indices[e] * CT], v1 = f[(int64_t)a.indices[e + 1] * CT];
            const double v2 = f[(int64_t)a.indices[e + 2] * CT], v3 = f[(int64_t)a.indices[e + 3] * CT];
            acc = acc + s0 * v0;
            acc = acc + s1 * v1;
            acc = acc + s2 * v2;
            acc = acc + s3 * v3;
        }
        for (; e < re; ++e) acc = acc + (-a.lap[e] * f[(int64_t)a.indices[e] * CT]);
        a.fout[row * CT + c] = a.alpha * acc;
    }
}

// The seeds of a chunk, one thread each.  init: f(0) = y on a zeroed buffer; else the second half of a step:
// f <- fl(f + fl((1 - alpha) y)) over what the step kernel wrote.  The (item, column) pairs of a chunk are distinct.
__global__ __launch_bounds__(DIF_THREADS) void diffuse_seed_kernel(const int32_t* __restrict__ item, const int32_t* __restrict__ col,
                                                                   const double* __restrict__ val, int64_t ns, double* f, int C, double om,
                                                                   int init) {
    for (int64_t t = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; t < ns; t += (int64_t)gridDim.x * DIF_THREADS) {
        double* cell = f + (int64_t)item[t] * C + col[t];
        *cell = init ? val[t] : *cell + om * val[t];
    }
}

// out[c][j] = f[ids[j]][c], c < nc, j < m (ids null: position == item): the [rows][m] layout the selection and the copies read
__global__ __launch_bounds__(DIF_THREADS) void diffuse_gather_kernel(const double* __restrict__ f, int C, int nc, const int32_t* __restrict__ ids,
                                                                     int64_t m, double* __restrict__ out) {
    for (int64_t j = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; j < m; j += (int64_t)gridDim.x * DIF_THREADS) {
        const double* row = f + (int64_t)(ids ? ids[j] : j) * C;
        for (int c = 0; c < nc; ++c) out[(int64_t)c * m + j] = row[c];
    }
}

// ------------------------------------------------------------------ host side
static std::atomic<int> g_diffuse_timing{0};
static std::atomic<int> g_diffuse_mib{DIF_MIB_DEFAULT};
static std::atomic<int> g_diffuse_cols{64};
static std::atomic<int> g_diffuse_tile{DIF_TILE_DEFAULT};
static std::atomic<int> g_diffuse_grid_cap{0};
void set_diffuse_timing(int v) { g_diffuse_timing.store(v ? 1 : 0, std::memory_order_relaxed); }
void set_diffuse_mib(int v) { g_diffuse_mib.store(v > 0 ? v : DIF_MIB_DEFAULT, std::memory_order_relaxed); }
void set_diffuse_cols(int v) { g_diffuse_cols.store(v > 0 ? v : 64, std::memory_order_relaxed); }
void set_diffuse_tile_edges(int v) { g_diffuse_tile.store(v > 0 ? std::min(v, DIF_TILE_MAX) : DIF_TILE_DEFAULT, std::memory_order_relaxed); }
void set_diffuse_grid_cap(int v) { g_diffuse_grid_cap.store(v > 0 ? v : 0, std::memory_order_relaxed); }

unsigned diffuse_grid(int64_t blocks) {
    const int64_t cap = g_diffuse_grid_cap.load(std::memory_order_relaxed);
    blocks = std::max<int64_t>(blocks, 1);
    return (unsigned)(cap > 0 ? std::min(blocks, cap) : blocks);
}

void diffuse_work_free(DiffuseWork* w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;   // (the buffers and the events free themselves)
}

double diffuse_kernel_us(const DiffuseWork* w) { return w ? w->kernel_us : 0.0; }
int diffuse_cols_cap() { return g_diffuse_cols.load(std::memory_order_relaxed); }
int diffuse_tile_edges() { return g_diffuse_tile.load(std::memory_order_relaxed); }
bool diffuse_timing() { return g_diffuse_timing.load(std::memory_order_relaxed) != 0; }

static as_status diffuse_work_create(const as_space* sp, DiffuseWork** out) {
    DiffuseWork* w = new (std::nothrow) DiffuseWork();
    if (!w) {
        set_err("diffuse: out of host memory");
        return AS_ENOMEM;
    }
    w->device = sp->device;
    if (hipDeviceGetAttribute(&w->cus, hipDeviceAttributeMultiprocessorCount, sp->device) != hipSuccess || w->cus <= 0) w->cus = 256;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking)) != hipSuccess || (e = w->ev.create()) != hipSuccess) {
        set_err("diffuse: creation of the stream and events failed: %s", hipGetErrorString(e));
        diffuse_work_free(w);
        return AS_EHIP;
    }
    *out = w;
    return AS_OK;
}

as_status diffuse_work_get(const as_space* sp, DiffuseWork** out) {
    if (!sp->diffuse_ws) AS_TRY(diffuse_work_create(sp, &sp->diffuse_ws));
    *out = sp->diffuse_ws;
    return AS_OK;
}

int diffuse_chunk_cols(int64_t rem, int64_t n, int cols_cap, int64_t budget, int bufs) {
    auto fits = [&](int c) { return c <= cols_cap && bufs * (int64_t)sizeof(double) * n * c <= budget; };
    if (rem > 32 && fits(64)) return 64;
    if (rem > 1 && fits(16)) return 16;
    return 1;
}

static void diffuse_step_launch(const DiffuseWork* w, const DiffuseArgs& a, int C) {
    if (C == 1) {
        const int64_t groups = (a.n + DIF_THREADS - 1) / DIF_THREADS;
        const unsigned grid = diffuse_grid(std::min<int64_t>(groups, (int64_t)w->cus * DIF_BLOCKS_PER_CU));
        hipLaunchKernelGGL(diffuse_step1_kernel, dim3(grid), dim3(DIF_THREADS), sizeof(double) * (size_t)a.tile, w->stream, a);
        return;
    }
    const int64_t per_block = (int64_t)(DIF_THREADS / 64) * (64 / C);   // rows of a block and trip
    const unsigned grid = diffuse_grid(std::min<int64_t>((a.n + per_block - 1) / per_block, (int64_t)w->cus * DIF_BLOCKS_PER_CU));
    if (C == 16) hipLaunchKernelGGL(diffuse_step_cols_kernel<16>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
    else hipLaunchKernelGGL(diffuse_step_cols_kernel<64>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, a);
}

as_status diffuse_frame(const as_space* sp, const as_graph* gr, const DiffuseCall& c, DiffuseFrame* fr) {
    try {
        for (int64_t i = 0; i < c.b; ++i)
            if (!c.served || c.served[i]) fr->q.push_back(i);
    } catch (const std::bad_alloc&) {
        set_err("diffuse: out of host memory for %lld queries", (long long)c.b);
        return AS_ENOMEM;
    }
    fr->select = c.sel != nullptr;
    fr->pick = !fr->select && c.pick_ids != nullptr;
    fr->m = fr->select || fr->pick ? c.m : gr->n;
    if (fr->q.empty() || gr->n <= 0 || fr->m <= 0) return AS_OK;
    if (!sp->diffuse_ws) AS_TRY(diffuse_work_create(sp, &sp->diffuse_ws));
    DiffuseWork* w = sp->diffuse_ws;
    fr->ids_d = fr->select ? c.pos_ids : nullptr;
    if (fr->pick) {
        AS_TRY(reserve_or_err(w->ids, fr->m, "diffuse listed ids"));
        AS_HIP(hipMemcpyAsync(w->ids, c.pick_ids, sizeof(int32_t) * (size_t)fr->m, hipMemcpyHostToDevice, w->stream));
        fr->ids_d = w->ids;
    }
    fr->w = w;
    return AS_OK;
}

as_status diffuse_seed_table(const DiffuseFrame& fr, const DiffuseCall& c, int64_t i0, int64_t nc, DiffuseSeeds* s) {
    DiffuseWork* w = fr.w;
    const std::vector<int64_t>& q = fr.q;
    int64_t ns = 0;
    for (int64_t t = 0; t < nc; ++t) ns += c.offs[q[i0 + t] + 1] - c.offs[q[i0 + t]];
    const size_t item_off = sizeof(double) * (size_t)ns, col_off = item_off + sizeof(int32_t) * (size_t)ns;
    const size_t up = col_off + sizeof(int32_t) * (size_t)ns;
    if (up > std::min(w->seed_d.size(), w->seed_h.size())) {
        AS_TRY(reserve_or_err(w->seed_d, up + up / 2, "diffuse seed table"));
        AS_TRY(reserve_or_err(w->seed_h, up + up / 2, "diffuse pinned seed table"));
    }
    char* const sh = w->seed_h;
    char* const sd = w->seed_d;
    double* hv = (double*)sh;
    int32_t* hi = (int32_t*)(sh + item_off);
    int32_t* hc = (int32_t*)(sh + col_off);
    int64_t z = 0;
    for (int64_t t = 0; t < nc; ++t)
        for (int64_t e = c.offs[q[i0 + t]]; e < c.offs[q[i0 + t] + 1]; ++e, ++z) {
            hv[z] = c.vals[e];
            hi[z] = (int32_t)c.ids[e];
            hc[z] = (int32_t)t;
        }
    if (ns > 0) AS_HIP(hipMemcpyAsync(sd, sh, up, hipMemcpyHostToDevice, w->stream));
    s->ns = ns;
    s->val = (const double*)sd;
    s->item = (const int32_t*)(sd + item_off);
    s->col = (const int32_t*)(sd + col_off);
    s->grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ns + DIF_THREADS - 1) / DIF_THREADS, 1024));
    return AS_OK;
}

void diffuse_seed_launch(const DiffuseWork* w, const DiffuseSeeds& s, double* f, int C, double om, int init) {
    if (s.ns > 0) hipLaunchKernelGGL(diffuse_seed_kernel, dim3(s.grid), dim3(DIF_THREADS), 0, w->stream, s.item, s.col, s.val, s.ns, f, C, om, init);
}

as_status diffuse_emit(const DiffuseFrame& fr, const DiffuseCall& c, int64_t i0, int64_t nc, int C, const double* f, bool timing, double* us) {
    DiffuseWork* w = fr.w;
    const std::vector<int64_t>& q = fr.q;
    const int64_t m = fr.m;
    // the whole f in the [rows][m] layout, unless it has that layout already (one column, every item, in item order)
    const bool gather = !(C == 1 && !fr.ids_d);
    const double* res = f;   // [nc][m] after the gather
    if (gather) {
        AS_TRY(reserve_or_err(w->rows, nc * m, "diffuse gathered rows"));
        const unsigned ggrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((m + DIF_THREADS - 1) / DIF_THREADS, (int64_t)w->cus * 8));
        hipLaunchKernelGGL(diffuse_gather_kernel, dim3(ggrid), dim3(DIF_THREADS), 0, w->stream, f, C, (int)nc, fr.ids_d, m, (double*)w->rows);
        AS_HIP(hipGetLastError());
        res = w->rows;
    }
    if (!fr.select) {
        // (queries that follow one another in the call: one copy)
        bool run = true;
        for (int64_t t = 1; t < nc; ++t) run = run && q[i0 + t] == q[i0] + t;
        if (run) AS_HIP(hipMemcpyAsync(c.out_rows + q[i0] * m, res, sizeof(double) * (size_t)(nc * m), hipMemcpyDeviceToHost, w->stream));
        else
            for (int64_t t = 0; t < nc; ++t)
                AS_HIP(hipMemcpyAsync(c.out_rows + q[i0 + t] * m, res + t * m, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, w->stream));
    }
    AS_TRY(sync_add_elapsed(w->stream, timing, w->ev.e, us));
    if (fr.select) {
        // the selection runs on the handle's stream: f is complete (the wait above)
        const int64_t k = std::min<int64_t>(std::min<int64_t>(c.k, m), SUBSET_TOPK);
        AS_TRY(subset_select_rows_from(c.sel, res, c.pos_ids, m, m, k, nc));   // -> c.sel->out[t]; waits
        const SubsetOut* so = c.sel->out;
        for (int64_t t = 0; t < nc; ++t) {
            const int64_t i = q[i0 + t];
            AS_TRY(subset_list_out(so + t, k, c.out_idx + i * c.stride, c.out_score + i * c.stride, c.out_len + i));
        }
    }
    return AS_OK;
}

static as_status diffuse_chunks(const as_space* sp, const as_graph* gr, const DiffuseCall& c, int64_t* counts) {
    const int64_t n = gr->n;
    DiffuseFrame fr;
    AS_TRY(diffuse_frame(sp, gr, c, &fr));
    if (!fr.w) return AS_OK;
    DiffuseWork* w = fr.w;
    const bool timing = diffuse_timing();
    const int cols_cap = diffuse_cols_cap();
    const int64_t budget = (int64_t)g_diffuse_mib.load(std::memory_order_relaxed) << 20;
    const double om = 1.0 - c.alpha;
    w->kernel_us = 0.0;
    const int64_t nq = (int64_t)fr.q.size();
    for (int64_t i0 = 0; i0 < nq;) {
        const int C = diffuse_chunk_cols(nq - i0, n, cols_cap, budget, 2);
        const int64_t nc = std::min<int64_t>(C, nq - i0);
        for (int s = 0; s < 2; ++s) AS_TRY(reserve_or_err(w->f[s], n * C, "diffuse f buffers"));
        DiffuseSeeds sd;
        AS_TRY(diffuse_seed_table(fr, c, i0, nc, &sd));
        double* fin = w->f[0];
        double* fout = w->f[1];
        AS_HIP(hipMemsetAsync(fin, 0, sizeof(double) * (size_t)(n * C), w->stream));
        diffuse_seed_launch(w, sd, fin, C, om, 1);
        if (timing) AS_HIP(hipEventRecord(w->ev.e[0], w->stream));
        for (int64_t t = 0; t < c.steps; ++t) {
            DiffuseArgs a;
            a.indptr = gr->indptr; a.indices = gr->indices; a.lap = gr->lap; a.fin = fin; a.fout = fout; a.n = n; a.alpha = c.alpha;
            a.tile = diffuse_tile_edges();
            diffuse_step_launch(w, a, C);
            diffuse_seed_launch(w, sd, fout, C, om, 0);
            std::swap(fin, fout);
        }
        AS_HIP(hipGetLastError());
        if (timing) AS_HIP(hipEventRecord(w->ev.e[1], w->stream));
        counts[0] += 1;
        counts[1] += c.steps;
        counts[2] += sd.ns;
        AS_TRY(diffuse_emit(fr, c, i0, nc, C, fin, timing, &w->kernel_us));
        i0 += nc;
    }
    return AS_OK;
}

// (a failed run leaves nothing on the stream when the caller releases the lock)
as_status diffuse_run(const as_space* sp, const as_graph* gr, const DiffuseCall& c, int64_t* counts) {
    const as_status s = c.max_iters > 0 ? diffuse_solve_chunks(sp, gr, c, counts) : diffuse_chunks(sp, gr, c, counts);
    if (s != AS_OK && sp->diffuse_ws) (void)hipStreamSynchronize(sp->diffuse_ws->stream);
    return s;
}

}  // namespace as
