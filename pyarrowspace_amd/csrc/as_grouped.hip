// Grouped search: the best items of the best groups.  Every item carries a group (as_groups: the
// caller's int64 labels as dense group numbers, ascending label); the answer is the first n_groups groups by their best member and
// the first per_group members of each, everything by (score descending, index ascending).  The scores come from the filtered
// forms' score kernels (as_subset.hip), unchanged, and stay on the device.  This file picks, per row (query) and per SLOT, the
// largest 96-bit key sel_ord(score) : ~position that lies strictly below the slot's previous pick (group_pick_kernel, two
// launches per round: the 64-bit part by atomicMax, then the position by atomicMin among the positions that hold that maximum).
// Round 0: slot == group, nothing excluded -- every group's head.  The heads' scores are scattered into a collapsed score row
// (NaN elsewhere) and the filtered forms' exact selection over it names the best n_groups groups.  Rounds 1 .. per_group - 1: slot
// == rank of a selected group (slot_of_group, -1 for the others, which issue nothing).  One gather kernel turns the picks of the
// later rounds into (id, score); one copy and one wait finish the call.
// Entry points: as_api.hip (as_groups_create, as_search_grouped, as_search_grouped_batch, as_grouped_counters, as_grouped_kernel_us).
#include <algorithm>
#include <atomic>
#include <new>

#include "as_common.hpp"

namespace as {

constexpr int GP_THREADS = 256;
constexpr int GP_LDS_SLOTS = 1024;     // == SUBSET_TOPK: the most slots a later round has
constexpr int GP_BLOCKS_PER_CU = 8;    // the grid: that many blocks per CU and row at most, the rest is the wave-stride loop

struct GroupPickArgs {
    const double* scores;                // [rows][ld]
    int64_t ld, m;
    const int32_t* ids;                  // [m] the subset's ids (position -> item)
    const int32_t* dense;                // [nitems] item -> group
    const int32_t* slot_of_group;        // later rounds: [rows][G], -1 for a group that was not selected
    int64_t G;
    unsigned long long* cell_hi;         // this round's cells, row r at + r * cells_ld: the largest 64-bit key part per slot (0: none)
    unsigned int* cell_pos;              // ... and the smallest position that holds it
    const unsigned long long* prev_hi;   // later rounds: the previous round's cells, same stride
    const unsigned int* prev_pos;
    int64_t cells_ld;
    int nslots;                          // slots of a row this round: G, or n_groups (the COMBINE form needs <= GP_LDS_SLOTS)
    unsigned long long* natom;           // pass A: 64-bit max-atomics issued, one atomicAdd per block
};

// One pass over the m positions of row blockIdx.y.  A wave's trip covers 64 consecutive positions, lane t position base + t.  Lanes
// with the same slot as their left neighbour form a RUN; a run's keys are combined by a segmented shuffle scan and its last lane
// issues ONE atomic -- a document's chunks are stored consecutively, so a wave issues one atomic per document it touches, not one
// per lane.  A lane whose key is out (a NaN score, or not below the slot's previous pick) keeps its slot and contributes the
// neutral key 0, so it never splits a run.
// Pass A: atomicMax of the run's largest key part; a plain read of the cell first skips an atomic that cannot win (the cell only
// grows during the pass: a stale read costs an atomic, never a result).  COMBINE (pass A with at most GP_LDS_SLOTS slots: every
// later round, round 0 of few groups): the runs' maxima go to a per-block table in LDS by LDS atomics and the block issues at most
// one global atomic per slot at its end -- few large interleaved groups would otherwise send every run of every wave to the same
// few addresses.  Pass B: the cell is final; the FIRST lane of a run whose key part equals it issues atomicMin of its position
// (positions ascend with the lane).
template <bool ROUND0, bool PASS_B, bool COMBINE>
__global__ __launch_bounds__(GP_THREADS) void group_pick_kernel(GroupPickArgs a) {
    __shared__ unsigned int wcount[GP_THREADS / WAVE];
    __shared__ unsigned long long lmax[COMBINE ? GP_LDS_SLOTS : 1];
    if (COMBINE) {
        for (int s = threadIdx.x; s < a.nslots; s += GP_THREADS) lmax[s] = 0ull;
        __syncthreads();
    }
    const int64_t row = blockIdx.y;
    const double* __restrict__ sc = a.scores + row * a.ld;
    unsigned long long* chi = a.cell_hi + row * a.cells_ld;
    unsigned int* cpos = a.cell_pos + row * a.cells_ld;
    const int lane = lane_id();
    const int64_t nwaves = (int64_t)gridDim.x * (GP_THREADS / WAVE);
    unsigned int issued = 0;   // (wave-uniform)
    for (int64_t base = ((int64_t)blockIdx.x * (GP_THREADS / WAVE) + (threadIdx.x >> 6)) * WAVE; base < a.m; base += nwaves * WAVE) {
        const int64_t p = base + lane;   // (base is wave-uniform: every lane takes every trip, the shuffles see all 64)
        int slot = -1;
        unsigned long long key = 0ull;
        if (p < a.m) {
            const int g = a.dense[a.ids[p]];
            slot = ROUND0 ? g : a.slot_of_group[row * a.G + g];
            if (slot >= 0) {
                key = sel_ord(sc[p]);
                if (!ROUND0 && key) {
                    const unsigned long long ph = a.prev_hi[row * a.cells_ld + slot];
                    const unsigned int pp = a.prev_pos[row * a.cells_ld + slot];
                    if (!(key < ph || (key == ph && (unsigned int)p > pp))) key = 0ull;   // not strictly below the previous pick
                }
            }
        }
        const int left = __shfl_up(slot, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || slot != left);
        const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // the run's first lane (bit 0 is always set)
        if (!PASS_B) {
            unsigned long long v = key;   // inclusive segmented max scan: the run's last lane ends with the run's maximum
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long u = __shfl_up(v, o, 64);
                if (lane - o >= start && u > v) v = u;
            }
            const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
            bool issue = tail && v != 0ull;   // (v != 0 implies slot >= 0)
            if (COMBINE) {
                if (issue && slot < a.nslots) atomicMax(&lmax[slot], v);
            } else {
                if (issue && chi[slot] >= v) issue = false;
                if (issue) atomicMax(&chi[slot], v);
                issued += (unsigned int)__popcll(__ballot(issue));
            }
        } else {
            const bool cand = key != 0ull && key == chi[slot];
            const unsigned long long cands = __ballot(cand);
            const unsigned long long before = ((1ull << lane) - 1ull) & ~((1ull << start) - 1ull);   // the run's lanes left of this one
            if (cand && !(cands & before)) atomicMin(&cpos[slot], (unsigned int)p);
        }
    }
    if (!PASS_B) {
        if (COMBINE) {
            __syncthreads();
            for (int s0 = 0; s0 < a.nslots; s0 += GP_THREADS) {   // (block-uniform trips: the ballot sees whole waves)
                const int s = s0 + threadIdx.x;
                const unsigned long long v = s < a.nslots ? lmax[s] : 0ull;
                const bool issue = v != 0ull && chi[s] < v;
                if (issue) atomicMax(&chi[s], v);
                issued += (unsigned int)__popcll(__ballot(issue));
            }
        }
        if (lane == 0) wcount[threadIdx.x >> 6] = issued;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int s = 0;
#pragma unroll
            for (int i = 0; i < GP_THREADS / WAVE; ++i) s += wcount[i];
            if (s) atomicAdd(a.natom, (unsigned long long)s);
        }
    }
}

// collapsed[row][head position of group g] = that head's score, for every group g < G of row blockIdx.y that has a member; the
// host has filled the rows with NaN (all-ones bytes) before
__global__ __launch_bounds__(GP_THREADS) void group_collapse_kernel(const double* __restrict__ scores, int64_t ld, int64_t m, int64_t G,
                                                                    const unsigned long long* __restrict__ cell_hi,
                                                                    const unsigned int* __restrict__ cell_pos, double* __restrict__ collapsed) {
    const int64_t row = blockIdx.y;
    for (int64_t g = (int64_t)blockIdx.x * GP_THREADS + threadIdx.x; g < G; g += (int64_t)gridDim.x * GP_THREADS) {
        if (cell_hi[row * G + g] == 0ull) continue;
        const unsigned int pos = cell_pos[row * G + g];
        if ((int64_t)pos < m) collapsed[row * m + pos] = scores[row * ld + pos];
    }
}

// the later rounds' tables of row blockIdx.y from the selected groups sel_group[row][ng] (rank order, -1 behind the last):
// slot_of_group[row][g] = rank (the host has set the rows to -1), and the round-0 cells of g as round 0 of the picks
__global__ __launch_bounds__(GP_THREADS) void group_slots_kernel(const int32_t* __restrict__ sel_group, int ng, int64_t G, int R,
                                                                 const unsigned long long* __restrict__ cell_hi,
                                                                 const unsigned int* __restrict__ cell_pos, int32_t* __restrict__ slot_of_group,
                                                                 unsigned long long* __restrict__ pick_hi, unsigned int* __restrict__ pick_pos) {
    const int64_t row = blockIdx.y;
    for (int s = blockIdx.x * GP_THREADS + threadIdx.x; s < ng; s += gridDim.x * GP_THREADS) {
        const int g = sel_group[row * ng + s];
        if (g < 0 || g >= G) continue;   // (the picks' rows were set to "none" with the cells)
        slot_of_group[row * G + g] = s;
        pick_hi[row * R * ng + s] = cell_hi[row * G + g];
        pick_pos[row * R * ng + s] = cell_pos[row * G + g];
    }
}

// (id, score) of the picks of rounds 1 .. R - 1 of row blockIdx.y: entry [row][r - 1][s]; id -1: that slot found no member
__global__ __launch_bounds__(GP_THREADS) void group_gather_kernel(const double* __restrict__ scores, int64_t ld, int64_t m,
                                                                  const int32_t* __restrict__ ids, int ng, int R,
                                                                  const unsigned long long* __restrict__ pick_hi,
                                                                  const unsigned int* __restrict__ pick_pos, double* __restrict__ res_score,
                                                                  int32_t* __restrict__ res_idx) {
    const int64_t row = blockIdx.y;
    const int per = (R - 1) * ng;
    for (int e = blockIdx.x * GP_THREADS + threadIdx.x; e < per; e += gridDim.x * GP_THREADS) {
        const int64_t cell = row * R * ng + ng + e;   // round 1 + e / ng, slot e % ng
        const unsigned int pos = pick_pos[cell];
        const bool have = pick_hi[cell] != 0ull && (int64_t)pos < m;
        res_idx[row * per + e] = have ? ids[pos] : -1;
        res_score[row * per + e] = have ? scores[row * ld + pos] : 0.0;
    }
}

// ------------------------------------------------------------------ host side
static std::atomic<int> g_grouped_timing{0};
void set_grouped_timing(int v) { g_grouped_timing.store(v ? 1 : 0, std::memory_order_relaxed); }

struct GroupedWork {
    dev_buf<unsigned long long> cell_hi;   // [rows][G] round 0
    dev_buf<unsigned int> cell_pos;
    dev_buf<double> collapsed;             // [rows][m]
    dev_buf<int32_t> slot_of_group;        // [rows][G]
    dev_buf<unsigned long long> pick_hi;   // [rows][R][ng]: round r's cells, round 0 copied from the groups' cells
    dev_buf<unsigned int> pick_pos;
    dev_buf<int32_t> sel_group;            // [rows][ng]
    pin_buf<int32_t> hsel_group;
    dev_buf<double> res;                   // [rows][R - 1][ng] scores, then as many int32 ids
    pin_buf<double> hres;
    dev_buf<unsigned long long> natom;     // [1]
    pin_buf<unsigned long long> hnatom;    // [2]: after round 0, at the end
    dev_events<4> ev;                      // made by the first call under "grouped_timing": round 0, the later rounds
};

void grouped_work_free(GroupedWork* g) { delete g; }

int64_t grouped_row_bytes(const as_groups* g, int64_t m, int64_t n_groups, int64_t per_group) {
    return m * (int64_t)sizeof(double) + g->count * 16 + n_groups * per_group * 24 + n_groups * 4;
}

static unsigned pick_grid(const SubsetWork* w, int64_t m) {
    return (unsigned)filtered_grid(std::max<int64_t>(1, std::min<int64_t>((m + GP_THREADS - 1) / GP_THREADS, (int64_t)w->cus * GP_BLOCKS_PER_CU)));
}

template <bool ROUND0>
static as_status pick_round(GroupedCall* c, const GroupPickArgs& a, int64_t rows) {
    const dim3 grid(pick_grid(c->w, c->m), (unsigned)rows);
    if (a.nslots <= GP_LDS_SLOTS) hipLaunchKernelGGL((group_pick_kernel<ROUND0, false, true>), grid, dim3(GP_THREADS), 0, c->w->stream, a);
    else hipLaunchKernelGGL((group_pick_kernel<ROUND0, false, false>), grid, dim3(GP_THREADS), 0, c->w->stream, a);
    hipLaunchKernelGGL((group_pick_kernel<ROUND0, true, false>), grid, dim3(GP_THREADS), 0, c->w->stream, a);
    AS_HIP(hipGetLastError());
    c->counts[0] += 2;
    c->counts[1] += 2 * rows * c->m;
    return AS_OK;
}

// Pass A of round 0 alone, for late-interaction search (as_maxsim.hip): cells[row][g] <- the largest sel_ord key of group g among
// the m positions of row `row` of scores ([rows][ld]); the caller has zeroed the cells (0: no member) and *natom counts the global
// max-atomics issued.  The COMBINE form where the groups fit its table, else the plain form -- the choice pick_round makes.
as_status group_max_launch(SubsetWork* w, const as_groups* gs, const double* scores, int64_t ld, int64_t m, int64_t rows,
                           unsigned long long* cells, unsigned long long* natom) {
    if (rows <= 0 || m <= 0) return AS_OK;
    GroupPickArgs a;
    a.scores = scores; a.ld = ld; a.m = m; a.ids = w->ids; a.dense = gs->dense_dev; a.slot_of_group = nullptr; a.G = gs->count;
    a.cell_hi = cells; a.cell_pos = nullptr; a.prev_hi = nullptr; a.prev_pos = nullptr; a.cells_ld = gs->count;
    a.nslots = (int)std::min<int64_t>(gs->count, 0x7fffffff); a.natom = natom;
    const dim3 grid(pick_grid(w, m), (unsigned)rows);
    if (a.nslots <= GP_LDS_SLOTS) hipLaunchKernelGGL((group_pick_kernel<true, false, true>), grid, dim3(GP_THREADS), 0, w->stream, a);
    else hipLaunchKernelGGL((group_pick_kernel<true, false, false>), grid, dim3(GP_THREADS), 0, w->stream, a);
    AS_HIP(hipGetLastError());
    return AS_OK;
}

as_status grouped_rows(GroupedCall* c, int64_t i0, int64_t rows, const double* scores, int64_t ld) {
    SubsetWork* w = c->w;
    const as_groups* gs = c->g;
    const int64_t m = c->m, G = gs->count, ng = c->n_groups, pg = c->per_group;
    if (rows <= 0 || m <= 0) return AS_OK;
    if (!w->grouped) {
        w->grouped = new (std::nothrow) GroupedWork();
        if (!w->grouped) {
            set_err("grouped: out of host memory");
            return AS_ENOMEM;
        }
    }
    GroupedWork* gw = w->grouped;
    hipStream_t st = w->stream;
    const bool timing = g_grouped_timing.load(std::memory_order_relaxed) != 0;
    if (timing && !gw->ev.e[3]) AS_HIP(gw->ev.create());
    AS_TRY(reserve_or_err(gw->cell_hi, rows * G, "grouped cells"));
    AS_TRY(reserve_or_err(gw->cell_pos, rows * G, "grouped position cells"));
    AS_TRY(reserve_or_err(gw->collapsed, rows * m, "grouped collapsed scores"));
    AS_TRY(reserve_or_err(gw->natom, 1, "grouped counter"));
    AS_TRY(reserve_or_err(gw->hnatom, 2, "grouped pinned counter"));
    unsigned long long* cell_hi = gw->cell_hi;
    unsigned int* cell_pos = gw->cell_pos;
    double* collapsed = gw->collapsed;
    unsigned long long* natom = gw->natom;
    unsigned long long* hnatom = gw->hnatom;

    // ---- round 0: every group's head, the collapsed row, the selection of the best groups
    AS_HIP(hipMemsetAsync(cell_hi, 0, sizeof(unsigned long long) * (size_t)(rows * G), st));
    AS_HIP(hipMemsetAsync(cell_pos, 0xff, sizeof(unsigned int) * (size_t)(rows * G), st));
    AS_HIP(hipMemsetAsync(collapsed, 0xff, sizeof(double) * (size_t)(rows * m), st));   // all-ones bytes: a NaN
    AS_HIP(hipMemsetAsync(natom, 0, sizeof(unsigned long long), st));
    GroupPickArgs a;
    a.scores = scores; a.ld = ld; a.m = m; a.ids = w->ids; a.dense = gs->dense_dev; a.slot_of_group = nullptr; a.G = G;
    a.cell_hi = cell_hi; a.cell_pos = cell_pos; a.prev_hi = nullptr; a.prev_pos = nullptr; a.cells_ld = G; a.nslots = (int)std::min<int64_t>(G, 0x7fffffff); a.natom = natom;
    if (timing) AS_HIP(hipEventRecord(gw->ev.e[0], st));
    AS_TRY(pick_round<true>(c, a, rows));
    if (timing) AS_HIP(hipEventRecord(gw->ev.e[1], st));
    const dim3 cgrid(pick_grid(w, G), (unsigned)rows);
    hipLaunchKernelGGL(group_collapse_kernel, cgrid, dim3(GP_THREADS), 0, st, scores, ld, m, G, (const unsigned long long*)cell_hi,
                       (const unsigned int*)cell_pos, collapsed);
    AS_HIP(hipGetLastError());
    AS_HIP(hipMemcpyAsync(hnatom, natom, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    const int64_t k = std::min<int64_t>(ng, m);
    int64_t one_idx[SUBSET_TOPK], one_len = 0;
    double one_score[SUBSET_TOPK];
    if (c->status) AS_TRY(subset_select_rows_from(w, collapsed, w->ids, m, m, k, rows));   // -> w->out[row]; waits
    else AS_TRY(subset_select_from(w, collapsed, m, k, one_idx, one_score, &one_len));
    if (timing) {
        float ms = 0.0f;
        AS_HIP(hipEventElapsedTime(&ms, gw->ev.e[0], gw->ev.e[1]));
        c->us += (double)ms * 1e3;
    }
    unsigned long long atoms = hnatom[0];

    // ---- the heads on the host: entries that came back NaN lie behind the last group that exists
    auto head_idx = [&](int64_t t, int64_t s) { return c->status ? ((const SubsetOut*)w->out)[t].idx[s] : one_idx[s]; };
    auto head_score = [&](int64_t t, int64_t s) { return c->status ? ((const SubsetOut*)w->out)[t].score[s] : one_score[s]; };
    auto served = [&](int64_t t) { return !c->status || c->status[i0 + t] != AS_EZEROLAMBDA; };
    int64_t R = 1;   // rounds to run: no selected group of a served row has more members than that
    for (int64_t t = 0; t < rows; ++t) {
        const int64_t i = i0 + t;
        c->out_ngroups[i] = 0;
        if (!served(t)) continue;
        if (c->status && ((const SubsetOut*)w->out)[t].len != k) {
            set_err("grouped: the selection returned %lld of %lld entries", (long long)((const SubsetOut*)w->out)[t].len, (long long)k);
            return AS_EHIP;
        }
        int64_t nsel = 0;
        for (; nsel < k; ++nsel) {
            const double v = head_score(t, nsel);
            if (v != v) break;
            const int64_t id = head_idx(t, nsel);
            if (id < 0 || id >= gs->n) {
                set_err("grouped: the selection returned item %lld", (long long)id);
                return AS_EHIP;
            }
            const int32_t g = gs->dense[(size_t)id];
            c->out_label[i * ng + nsel] = gs->labels[(size_t)g];
            c->out_count[i * ng + nsel] = 1;
            c->out_idx[(i * ng + nsel) * pg] = id;
            c->out_score[(i * ng + nsel) * pg] = v;
            R = std::max<int64_t>(R, std::min<int64_t>(pg, gs->size[(size_t)g]));
        }
        c->out_ngroups[i] = nsel;
        c->counts[3] += nsel;
        c->counts[4] += nsel;
    }

    // ---- rounds 1 .. R - 1 over the selected groups
    if (R > 1) {
        const int64_t per = (R - 1) * ng, words = rows * per + (rows * per + 1) / 2;
        AS_TRY(reserve_or_err(gw->slot_of_group, rows * G, "grouped slot table"));
        AS_TRY(reserve_or_err(gw->pick_hi, rows * R * ng, "grouped picks"));
        AS_TRY(reserve_or_err(gw->pick_pos, rows * R * ng, "grouped pick positions"));
        AS_TRY(reserve_or_err(gw->sel_group, rows * ng, "grouped selected groups"));
        AS_TRY(reserve_or_err(gw->hsel_group, rows * ng, "grouped pinned selected groups"));
        AS_TRY(reserve_or_err(gw->res, words, "grouped result"));
        AS_TRY(reserve_or_err(gw->hres, words, "grouped pinned result"));
        int32_t* hsel = gw->hsel_group;
        for (int64_t t = 0; t < rows; ++t) {
            const int64_t nsel = served(t) ? c->out_ngroups[i0 + t] : 0;
            for (int64_t s = 0; s < ng; ++s) hsel[t * ng + s] = s < nsel ? gs->dense[(size_t)head_idx(t, s)] : -1;
        }
        int32_t* sel_group = gw->sel_group;
        int32_t* slot_of_group = gw->slot_of_group;
        unsigned long long* pick_hi = gw->pick_hi;
        unsigned int* pick_pos = gw->pick_pos;
        double* res_score = gw->res;
        int32_t* res_idx = (int32_t*)(res_score + rows * per);
        AS_HIP(hipMemcpyAsync(sel_group, hsel, sizeof(int32_t) * (size_t)(rows * ng), hipMemcpyHostToDevice, st));
        AS_HIP(hipMemsetAsync(slot_of_group, 0xff, sizeof(int32_t) * (size_t)(rows * G), st));   // -1
        AS_HIP(hipMemsetAsync(pick_hi, 0, sizeof(unsigned long long) * (size_t)(rows * R * ng), st));
        AS_HIP(hipMemsetAsync(pick_pos, 0xff, sizeof(unsigned int) * (size_t)(rows * R * ng), st));
        const dim3 sgrid((unsigned)((ng + GP_THREADS - 1) / GP_THREADS), (unsigned)rows);
        hipLaunchKernelGGL(group_slots_kernel, sgrid, dim3(GP_THREADS), 0, st, (const int32_t*)sel_group, (int)ng, G, (int)R,
                           (const unsigned long long*)cell_hi, (const unsigned int*)cell_pos, slot_of_group, pick_hi, pick_pos);
        AS_HIP(hipGetLastError());
        if (timing) AS_HIP(hipEventRecord(gw->ev.e[2], st));
        for (int64_t r = 1; r < R; ++r) {
            a.slot_of_group = slot_of_group;
            a.cell_hi = pick_hi + r * ng; a.cell_pos = pick_pos + r * ng;
            a.prev_hi = pick_hi + (r - 1) * ng; a.prev_pos = pick_pos + (r - 1) * ng;
            a.cells_ld = R * ng;
            a.nslots = (int)ng;
            AS_TRY(pick_round<false>(c, a, rows));
        }
        if (timing) AS_HIP(hipEventRecord(gw->ev.e[3], st));
        const dim3 ggrid((unsigned)((per + GP_THREADS - 1) / GP_THREADS), (unsigned)rows);
        hipLaunchKernelGGL(group_gather_kernel, ggrid, dim3(GP_THREADS), 0, st, scores, ld, m, (const int32_t*)w->ids, (int)ng, (int)R,
                           (const unsigned long long*)pick_hi, (const unsigned int*)pick_pos, res_score, res_idx);
        AS_HIP(hipGetLastError());
        AS_HIP(hipMemcpyAsync(gw->hres, res_score, sizeof(double) * (size_t)(rows * per) + sizeof(int32_t) * (size_t)(rows * per),
                              hipMemcpyDeviceToHost, st));
        AS_HIP(hipMemcpyAsync(hnatom + 1, natom, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        AS_HIP(hipStreamSynchronize(st));
        if (timing) {
            float ms = 0.0f;
            AS_HIP(hipEventElapsedTime(&ms, gw->ev.e[2], gw->ev.e[3]));
            c->us += (double)ms * 1e3;
        }
        atoms = hnatom[1];
        const double* hscore = gw->hres;
        const int32_t* hidx = (const int32_t*)(hscore + rows * per);
        for (int64_t t = 0; t < rows; ++t) {
            if (!served(t)) continue;
            const int64_t i = i0 + t;
            for (int64_t s = 0; s < c->out_ngroups[i]; ++s) {
                int64_t cnt = 1;
                for (int64_t r = 1; r < R; ++r, ++cnt) {
                    const int64_t e = t * per + (r - 1) * ng + s;
                    if (hidx[e] < 0) break;   // a slot without a member in a round has none in the rounds behind it
                    c->out_idx[(i * ng + s) * pg + r] = hidx[e];
                    c->out_score[(i * ng + s) * pg + r] = hscore[e];
                }
                c->out_count[i * ng + s] = cnt;
                c->counts[4] += cnt - 1;
            }
        }
    }
    c->counts[2] += (int64_t)atoms;
    return AS_OK;
}

}  // namespace as
