// What the diffusion files share (as_diffuse.hip: the S19 recurrence; as_diffuse_solve.hip: the S20 conjugate-gradient solve of
// its fixed point; as_spectral.hip: the S21 eigenpairs, which use the four blocks and the partials; as_components.hip: the S22
// connected components, on buffers of their own): the work buffers of a space, the column-chunk rule, the sparse seed table and its kernel, and the output
// paths (gather, selection on the handle's stream, score pick, raw block).  Defined in as_diffuse.hip.
#pragma once
#include <vector>

#include "as_common.hpp"

namespace as {

constexpr int DIF_THREADS = 256;          // threads of a block: the rows of a group of the C = 1 kernels
constexpr int DIF_TILE_DEFAULT = 4096;    // edges of an LDS tile of the C = 1 kernels ("diffuse_tile_edges"): 32 KiB of products
constexpr int DIF_TILE_MAX = 4096;
constexpr int DIF_BLOCKS_PER_CU = 8;
// "diffuse_mib", the budget of the two f buffers: 64 columns at 1M rows (977 MiB) -- measured 1.6x faster per query-step there than
// 16 columns (section 5.22), although that block no longer fits the Infinity Cache
constexpr int DIF_MIB_DEFAULT = 1024;
// "diffuse_solve_mib", the budget of the solve's four vectors: twice the above, so the column widths per N are the recurrence's
constexpr int DIF_SOLVE_MIB_DEFAULT = 2 * DIF_MIB_DEFAULT;
constexpr int DIF_SOLVE_COLS = 64;        // the stride of the solve's per-column scalars: the widest chunk
// "spectral_mib", the budget of the eigensolver's four blocks: 64 columns up to 4M rows.  A choice, not a measurement.
constexpr int SPC_MIB_DEFAULT = 8192;

struct DiffuseWork {
    int device = 0;
    int cus = 256;
    hipStream_t stream = nullptr;
    dev_buf<double> f[2];       // [n][C] each: the recurrence's ping-pong pair; the solve's x and r
    dev_buf<double> rows;       // [nc][m]: the last step's output, gathered
    dev_buf<int32_t> ids;       // the listed ids of a score call
    dev_buf<char> seed_d;       // one upload per chunk: [ns] values, [ns] items, [ns] columns
    pin_buf<char> seed_h;
    dev_events<2> ev;
    double kernel_us = 0.0;     // the steps (step and seed kernels) summed over the chunks of the last timed call
    // the solve (S20): p and q beside f[0] = x and f[1] = r, the segment partials of a dot, the columns' scalars and their pinned copy
    dev_buf<double> sv[2];      // [n][C] each: p, q
    dev_buf<double> part;       // [ceil(n / 64)][C]
    dev_buf<char> scal_d;       // SolveScalars (as_diffuse_solve.hip)
    pin_buf<char> scal_h;
    double solve_us = 0.0;      // first to last launch of the iterations, summed over the chunks of the last timed solve
    double solve_part_us[5] = {};   // ... and of one sampled iteration per chunk: apply, reduce of p.q, update, reduce of r.r, direction
    // the eigenpairs (S21): the four blocks are f[0..1] and sv[0..1], the partials of a Gram or of a column dot are `part`
    dev_buf<double> spec_d;     // [C][C] the matrix of a rotate, [C] the Ritz values behind it
    pin_buf<double> spec_h;     // the same pair, then a downloaded Gram [C][C] and the squared residual norms [C]
    dev_events<2> spec_ev;      // made by the first timed call
    // the last call: [0] its wall time; under "diffuse_timing" the device time of [1] steps, [2] Grams, [3] rotates, [4] colnorm2;
    // [5] the host's eigensolver, [6] the host's waits
    double spectral_us[7] = {};
    // the connected components (S22, as_components.hip): the labels' state, the sizes of the statistics, the words a stage leaves
    // (as_components.hip: CcStat) and their pinned copy
    dev_buf<int32_t> cc_parent;   // [n]
    dev_buf<int32_t> cc_size;     // [n]
    dev_buf<unsigned long long> cc_stat_d;
    pin_buf<unsigned long long> cc_stat_h;
    dev_events<3> cc_ev;          // made by the first timed call
    // the last call under "diffuse_timing": the device time of [0] its hooks, [1] its compress launches, [2] its statistics; [3] its rounds
    double cc_us[4] = {};
};

// the tunings both files honour
int diffuse_cols_cap();        // "diffuse_cols"
int diffuse_tile_edges();      // "diffuse_tile_edges"
bool diffuse_timing();         // "diffuse_timing"
unsigned diffuse_grid(int64_t blocks);   // "diffuse_grid_cap" clips a grid of `blocks`
// columns of the next chunk: `rem` served queries are left, n rows, at most `cols_cap` columns, `bufs` [n][C] buffers within `budget` bytes
int diffuse_chunk_cols(int64_t rem, int64_t n, int cols_cap, int64_t budget, int bufs);

// A call's frame: the served queries (ascending), the workspace, the ids the output gathers and the width of an output row
struct DiffuseFrame {
    std::vector<int64_t> q;
    DiffuseWork* w = nullptr;   // null: nothing to do (no served query, no item, no output position)
    const int32_t* ids_d = nullptr;
    int64_t m = 0;
    bool select = false, pick = false;
};
as_status diffuse_frame(const as_space* sp, const as_graph* gr, const DiffuseCall& c, DiffuseFrame* fr);
// the space's workspace, made on first use (under sp->fmu)
as_status diffuse_work_get(const as_space* sp, DiffuseWork** out);
// the seed table of the chunk fr->q[i0 .. i0 + nc): built in pinned memory and uploaded on the work's stream
struct DiffuseSeeds {
    int64_t ns = 0;
    const double* val = nullptr;
    const int32_t* item = nullptr;
    const int32_t* col = nullptr;
    unsigned grid = 1;
};
as_status diffuse_seed_table(const DiffuseFrame& fr, const DiffuseCall& c, int64_t i0, int64_t nc, DiffuseSeeds* s);
// diffuse_seed_kernel over the table (nothing with no seed).  init: f = y on a zeroed buffer; else f <- fl(f + fl(om y))
void diffuse_seed_launch(const DiffuseWork* w, const DiffuseSeeds& s, double* f, int C, double om, int init);
// the output of a chunk whose answer is f ([n][C], columns 0 .. nc): gather, then the raw / picked rows to the host or the selection
// on the handle's stream.  Waits for the work's stream; timing: adds ev[0] .. ev[1] to *us.
as_status diffuse_emit(const DiffuseFrame& fr, const DiffuseCall& c, int64_t i0, int64_t nc, int C, const double* f, bool timing, double* us);
// the S20 solve of a call with c.max_iters > 0 (as_diffuse_solve.hip): counts[0] += chunks, [1] += iterations launched, [2] += host
// waits of the iteration loop, [3] += seeds uploaded
as_status diffuse_solve_chunks(const as_space* sp, const as_graph* gr, const DiffuseCall& c, int64_t* counts);

}  // namespace as
