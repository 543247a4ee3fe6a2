/* arrowspace_hip.h -- C ABI of the MI355X-native hot path (gfx950).
 *
 * Drop-in boundary for the two calls the reference's PyO3 shim forwards to the
 * `arrowspace` crate:
 *     ArrowSpaceBuilder.build(graph_params, items)   /root/reference/src/lib.rs:271-300
 *     ArrowSpace.search(item, gl, tau)               /root/reference/src/lib.rs:132-174
 * plus the accessors the shim exposes (src/lib.rs:40-61, 78-124) and the debug
 * switch (src/helpers.rs:12-21).  Plain pointers and sizes only; no torch / numpy
 * types.  INTEGRATION.md shows the PyO3-side and ctypes-side bindings.
 *
 * Conventions
 *   - every function that can fail returns an as_status; 0 == AS_OK;
 *     as_last_error() returns a thread-local message for the last failure;
 *   - outputs are caller-allocated; handles are opaque and immutable after build;
 *   - AS_EINVAL maps to the shim's PyValueError, AS_EZEROLAMBDA to the
 *     `assert_ne!(lambda_q, 0.0)` panic at src/lib.rs:156-159, AS_EHIP to a
 *     runtime failure of the device / HIP runtime.
 *   - "host" pointers are ordinary CPU memory, "dev" pointers are HIP device memory
 *     on the device the handle lives on.
 */
#ifndef ARROWSPACE_HIP_H
#define ARROWSPACE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    AS_OK = 0,
    AS_EINVAL = 1,       /* bad argument            -> ValueError   */
    AS_EZEROLAMBDA = 2,  /* lambda_q == 0           -> PanicException (src/lib.rs:156-159) */
    AS_EHIP = 3,         /* HIP runtime failure     -> RuntimeError */
    AS_EUNSUPPORTED = 4, /* outside supported range -> ValueError   */
    AS_ENOMEM = 5
} as_status;

/* graph_params dict of the reference (src/helpers.rs:48-76).  has_sigma == 0
 * reproduces "sigma missing or None -> eps * 0.5" (src/helpers.rs:68-72). */
typedef struct {
    double eps;
    int64_t k;
    int64_t topk;
    double p;
    double sigma;
    int32_t has_sigma;
    int32_t _pad;
} as_graph_params;

enum { AS_METRIC_L2 = 0, AS_METRIC_COSINE = 1 };
enum { AS_KERNEL_GAUSSIAN = 0, AS_KERNEL_RATIONAL = 1 };
/* Which lambda the index carries.  ITEM: node-local spectral energy on the N-node item graph (BASELINE.json
 * north_star).  FEATURE: the synthetic index of the reference's notes -- a Rayleigh quotient and an edgewise
 * dispersion on an F x F feature-space Laplacian whose nodes are the D columns of the item matrix
 * (/root/reference/TAUMODE.md:8,12-27, GRAPH_VARIABLES.md:17); the GraphLaplacian is then that F x F object
 * (nnodes == nfeatures), the one `prepare_query_item(&v, gl)` takes the query's quotient against
 * (/root/reference/src/lib.rs:154). */
enum { AS_LAMBDA_ITEM = 0, AS_LAMBDA_FEATURE = 1 };
enum { AS_KEEP_F64_AUTO = 0, AS_KEEP_F64_ALWAYS = 1 };
enum { AS_DTYPE_F32 = 0, AS_DTYPE_F64 = 1 };

/* Options that have no counterpart in the reference's dict; zero-initialised ==
 * north_star defaults (L2 distance, Gaussian weights, current device). */
typedef struct {
    int32_t metric;   /* AS_METRIC_*  (cosine = GRAPH_VARIABLES.md:7 variant) */
    int32_t kernel;   /* AS_KERNEL_*  (rational = GRAPH_VARIABLES.md:9 variant) */
    int32_t device;   /* HIP device ordinal; -1 = current device */
    int32_t keep_f64; /* AS_KEEP_F64_*: AUTO keeps an fp64 copy of the items only when
                         they are not exactly representable in fp32 */
    int32_t force_exact; /* 1: skip the fp32 fast paths (fp64 everywhere; for tests) */
    int32_t search_mode; /* test hook: start searches on a fallback path (bit0 fp64, bit1 wavefront-list selection) */
    int32_t lambda_mode; /* AS_LAMBDA_* */
    int32_t reserved;
} as_opts;

typedef struct as_space as_space; /* crate `ArrowSpace`      (src/lib.rs:64-67)  */
typedef struct as_graph as_graph; /* crate `GraphLaplacian`  (src/lib.rs:26-29)  */
typedef struct as_query as_query; /* per-search device workspace (no reference counterpart) */

/* ---- index build: replaces RustBuilder::...build(rows), src/lib.rs:278-289 ---- */

/* items: host fp64, element strides (numpy `as_array()` accepts any strides,
 * src/helpers.rs:25).  n == 0 or d == 0 -> AS_EINVAL (src/helpers.rs:27-29). */
as_status as_build(const double* items, int64_t n, int64_t d, int64_t row_stride, int64_t col_stride,
                   const as_graph_params* gp, const as_opts* opts, as_space** out_space, as_graph** out_graph);

/* Same, items already resident in HBM (row-major, leading dimension ld elements).  Synchronises the device
 * first: whatever stream produced the items, they are complete when the ingest reads them. */
as_status as_build_dev(const void* items_dev, int32_t dtype, int64_t n, int64_t d, int64_t ld,
                       const as_graph_params* gp, const as_opts* opts, as_space** out_space, as_graph** out_graph);

/* ---- staged build: the three steps as_build composes; multi-GPU hosts call them
 *      with a row range per rank and all-gather the lists in between ---- */

/* step 1: ingest items into the HBM layout (fp32 padded tile layout + norms). */
as_status as_space_create_dev(const void* items_dev, int32_t dtype, int64_t n, int64_t d, int64_t ld,
                              const as_opts* opts, as_space** out_space);
/* step 2: exact directed k-NN lists for rows [row_begin, row_end) against all n items.
 * Outputs (device, caller-allocated, (row_end-row_begin) x k, row-major):
 *   out_idx int32 (-1 padded), out_key / out_dist / out_gy fp64, out_cnt int32 per row. */
as_status as_knn_rows(const as_space* sp, const as_graph_params* gp, int64_t row_begin, int64_t row_end,
                      int32_t* out_idx_dev, double* out_key_dev, double* out_dist_dev, double* out_gy_dev,
                      int32_t* out_cnt_dev);
/* step 3: symmetrise + normalised Laplacian + per-item energy + lambdas from the
 * complete n x k lists (device).  Writes lambdas into the space.
 * The lists are taken as as_knn_rows leaves them and are NOT validated (as_graph_from_knn_global alike): row i holds
 * cnt[i] <= k entries; every id is in [0, n), is not i, and occurs once in its row; slots past cnt[i] are never read,
 * whatever they hold.  An id outside [0, n) is an out-of-bounds access.  (as_graph_shard_csr checks its ids.) */
as_status as_graph_from_knn(as_space* sp, const as_graph_params* gp, const int32_t* idx_dev,
                            const double* dist_dev, const double* gy_dev, const int32_t* cnt_dev,
                            as_graph** out_graph);

/* ---- staged build without replication (row-sharded multi-GPU): a rank's space holds only ITS rows;
 *      the other ranks' shards visit one at a time as temporary spaces (ring send/recv in the host).  Per visiting
 *      block as_knn_block fills that block's slice of the partial lists (M = as_knn_list_width(k) exact entries per
 *      row, ids global); as_knn_merge ranks the slices of all blocks, applies eps and k and flags the rows for which
 *      something a block dropped could still belong to the answer; those rows go round once more through
 *      as_knn_block_band (complete collection inside the proven band), then as_knn_merge again.  Partial arrays are
 *      device memory, caller-allocated: key / dist / gy fp64 and idx int32 [nblocks][rows][M], cnt int32 and t32 fp32
 *      [nblocks][rows]; the pointers passed to as_knn_block / _band are those of ONE block's slice.
 *      A SLICE, per row: the low 16 bits of cnt = the number of entries (<= M), ordered by (key ascending, id ascending),
 *      no (key, id) pair twice; slots past the count are never read, and unspecified after a call.  Bits 16-29 of cnt are
 *      0.  Bit 30 = "this slice dropped or turned away something", and then t32 is a lower bound of the fp32 keys of what
 *      it dropped (-inf: no bound is known; the row fails its proof); without bit 30, t32 is not read.  Bit 30 and t32
 *      count whatever the number of entries: a slice that kept NO entry may still have turned candidates away (a gated
 *      transposed slice), and as_knn_fold and as_knn_merge both honour its bound.  Cutting exact entries beyond the M-th
 *      in a fold sets no bit (k <= M - 8: they cannot be among the k nearest).  A row is proven when, for every slice
 *      with bit 30, t32 - e > B strictly (B = its k-th key inside eps, or the eps key with fewer; e = the fp32 error term
 *      of the row against that block, 0 for a folded slice, whose t32 already carries it); equality, NaN and -inf flag
 *      the row.  tests/test_gpu_ring_lists.py states all of it against oracle/oracle_np.py. ---- */
int32_t as_knn_list_width(int64_t k);                 /* M; < 0 when k is not supported */
int32_t as_record_capacity(int32_t which);            /* 0: k-NN records a query merges (ranks x k); 1: hit records (ranks x (topk + 1)) */
double as_space_nmax(const as_space* sp);             /* largest squared norm (error bound of a block's dropped candidates) */
as_status as_space_norms(const as_space* sp, double* out_dev); /* fp64 squared norms of the space's rows, device to device */
int64_t as_space_row_offset(const as_space* sp);      /* Ring build: may the block passes (as_knn_block / _pair / _band) run on the int8 two-digit images of the shards?  Every rank
 * reports what its own rows measure -- out3 = {U, V, 1.0 when its image cannot be used (non-finite rows, ARROWSPACE_K2_NO_I8) else
 * 0.0} (as_ring_i8_stats makes the image) --, the host all-gathers the three numbers and hands every rank the ring-wide maxima:
 * as_ring_i8_set(sp, max U, max V, usable = no rank said 1).  usable = 0 or a coefficient 2.001 U + V^2 beyond 1e-3 keeps the
 * bf16 head + tail form, on every rank alike (as_ring_i8: what was decided).  Graphs are the same bits either way.
 * Serves ArrowSpaceBuilder::build, /root/reference/src/lib.rs:281-331, on a row-sharded index. */
as_status as_ring_i8_stats(as_space* sp, double* out3);
as_status as_ring_i8_set(as_space* sp, double u_max, double v_max, int32_t usable);
int32_t as_ring_i8(const as_space* sp);
/* global index of row 0 (set by as_graph_from_knn_global) */
as_status as_knn_block(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t row_begin, int64_t row_end,
                       int64_t row_goff, int64_t col_goff, double* p_key_dev, double* p_dist_dev, double* p_gy_dev,
                       int32_t* p_idx_dev, int32_t* p_cnt_dev, float* p_t32_dev);
/* Symmetric ring: an unordered pair of blocks is computed ONCE.  as_knn_block_pair runs the own rows
 * [row_begin, row_end) against the visiting block's column tiles [col_tile_begin, col_tile_end) (128 items each; -1 /
 * -1 = all) and lets every key serve both items: p_* is the own rows' slice exactly as as_knn_block's (indexed from
 * row_begin), q_* the slice of ALL visiting items [cols nitems][M] with the own rows as their columns (ids global),
 * refined here while both shards are resident, to be sent home and folded there (as_knn_fold with the sender's
 * block_nmax).  A visiting item's candidates are admitted up to min(eps bound, col_thr_dev[item]); q_t32 carries the
 * bound of what was turned away (-inf when its buffer overflowed: the item fails its proof and takes the second
 * round).  as_knn_thresholds derives such thresholds from a rank's folded list (an upper bound of each row's M-th
 * smallest fp32 key over all columns: its M-th exact key so far + the error bound; +inf while the list is not full);
 * nmax_all = the largest squared norm of the whole index.  row_thr_dev (may be NULL): the same kind of thresholds for the
 * OWN rows, indexed by the row's number in sp ([nitems]) -- a row then starts every unit from min(eps bound, threshold)
 * instead of the eps bound (an eps that admits every pair leaves only the thresholds to prune with).  Scratch: the
 * visiting block is taken in chunks of column
 * tiles whose transposed buffers (8 KiB per item at M = 64) fit in an eighth of the free memory, at most 16 GB. */
as_status as_knn_block_pair(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t row_begin, int64_t row_end,
                            int64_t col_tile_begin, int64_t col_tile_end, int64_t row_goff, int64_t col_goff,
                            const float* col_thr_dev, const float* row_thr_dev, double* p_key_dev, double* p_dist_dev, double* p_gy_dev,
                            int32_t* p_idx_dev, int32_t* p_cnt_dev, float* p_t32_dev, double* q_key_dev, double* q_dist_dev,
                            double* q_gy_dev, int32_t* q_idx_dev, int32_t* q_cnt_dev, float* q_t32_dev);
as_status as_knn_thresholds(const as_space* sp, const as_graph_params* gp, int64_t row_begin, int64_t row_end, double nmax_all,
                            const double* r_key_dev, const int32_t* r_cnt_dev, float* out_thr_dev);
as_status as_knn_merge(const as_space* sp, const as_graph_params* gp, int64_t row_begin, int64_t row_end, int32_t nblocks,
                       const double* p_key_dev, const double* p_dist_dev, const double* p_gy_dev, const int32_t* p_idx_dev,
                       const int32_t* p_cnt_dev, const float* p_t32_dev, const double* block_nmax_host, int32_t* out_idx_dev,
                       double* out_key_dev, double* out_dist_dev, double* out_gy_dev, int32_t* out_cnt_dev,
                       int32_t* out_flag_dev, double* out_band_dev, int64_t* out_nflagged);
/* Running fold (what dist.py uses: two slices of list memory whatever the number of ranks): r_* <- the M smallest exact
 * entries of r_* and b_* per row; r_t32 keeps min over blocks of (T32_b - e_b).  mode 0: every row; 1: rows with
 * flag_dev != 0; 2: those rows, their running list discarded first (first block of the second round).  as_knn_merge
 * with nblocks == 0 then finalises the one folded slice. */
as_status as_knn_fold(const as_space* sp, const as_graph_params* gp, int64_t row_begin, int64_t row_end, int32_t mode,
                      double block_nmax, const int32_t* flag_dev, double* r_key_dev, double* r_dist_dev, double* r_gy_dev,
                      int32_t* r_idx_dev, int32_t* r_cnt_dev, float* r_t32_dev, const double* b_key_dev, const double* b_dist_dev,
                      const double* b_gy_dev, const int32_t* b_idx_dev, const int32_t* b_cnt_dev, const float* b_t32_dev);
as_status as_knn_block_band(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t row_begin,
                            int64_t row_end, int64_t row_goff, int64_t col_goff, int32_t* flag_dev /* bit 1: band overflow */,
                            const double* band_dev, double* p_key_dev, double* p_dist_dev, double* p_gy_dev,
                            int32_t* p_idx_dev, int32_t* p_cnt_dev, float* p_t32_dev, int64_t* out_overflowed);
/* Last resort of the ring (third round): rows whose band overflowed the collection buffers somewhere (flag_dev != 0 --
 * thousands of exact duplicates, or of items at one distance) take the block's k nearest inside eps by exact evaluation
 * of every pair, ordered by (key, global id); the slice carries no drop bound.  Row-serial cost, as the last resort of
 * as_knn_rows (the reference's own loop is this for every row: the crate's all-pairs build, src/lib.rs:278-289). */
as_status as_knn_block_exact(const as_space* sp, const as_space* cols, const as_graph_params* gp, int64_t row_begin, int64_t row_end,
                             int64_t row_goff, int64_t col_goff, const int32_t* flag_dev, double* p_key_dev, double* p_dist_dev,
                             double* p_gy_dev, int32_t* p_idx_dev, int32_t* p_cnt_dev, float* p_t32_dev);
/* step 3 over the lists of ALL n_global items for a space that holds the rows [row_offset, row_offset + nitems):
 * global graph, Laplacian, energies, tau0; this shard's lambdas into the space.  n64_global_dev: fp64 squared norms
 * of all items (device).  Searches on the space then report global item ids.
 * Lists: n_global x k, under as_graph_from_knn's assumptions (ids in [0, n_global), no self, no repeat in a row,
 * cnt <= k, slots past cnt ignored) -- assumed, not checked. */
as_status as_graph_from_knn_global(as_space* sp, const as_graph_params* gp, int64_t n_global, int64_t row_offset,
                                   const int32_t* idx_dev, const double* dist_dev, const double* gy_dev,
                                   const int32_t* cnt_dev, const double* n64_global_dev, as_graph** out_graph);

/* Sharded graph stage, in front of the host's variable-count all-to-all: the directed edges i -> j of this rank's k-NN lists
 * (idx / dist / gy [rows][k], cnt[rows] valid entries per row; device pointers), bucketed by the rank that owns item j
 * (rank r owns [bounds_host[r], bounds_host[r + 1])): out_ints [E][2] int32 = (j - bounds[owner], row0 + i), out_reals [E][2]
 * = (dist, gy), buckets in rank order, the lists' (row, slot) order inside a bucket; out_counts_host[r] = entries for rank r.
 * The output buffers hold rows * k entries.  Count / scan / scatter kernels on `hip_stream`; synchronises it.
 * Serves ArrowSpaceBuilder::build, /root/reference/src/lib.rs:281-331, on a row-sharded index. */
as_status as_edges_bucket(const int32_t* idx_dev, const double* dist_dev, const double* gy_dev, const int32_t* cnt_dev, int64_t rows, int64_t k,
                          int64_t row0, const int64_t* bounds_host, int32_t world, int32_t* out_ints_dev, double* out_reals_dev,
                          int64_t* out_counts_host, void* hip_stream);
/* step 3 without replication (SURVEY 8e "Symmetrise + Laplacian": one exchange step).  The space holds the rows
 * [row_offset, row_offset + nitems); idx/dist/gy/cnt are ITS rows' lists (ids global).  in_*: the directed edges
 * (in_col_dev[e] -> row_offset + in_row_dev[e]) of ALL ranks whose target row lives here, this rank's own included
 * -- what the host's variable-count all-to-all delivers.  as_graph_shard_csr builds these rows of the symmetrised
 * graph (column ids global) and their degrees (as_graph_deg_copy: nitems doubles, device to device);
 * as_graph_shard_energy takes the degrees and squared norms of all items (all-gathered: 16 B per item) and leaves
 * the rows' energies behind (as_graph_energy_copy); as_graph_shard_lambdas takes the energies of all items (8 B per
 * item), selects tau0 over them and writes this shard's lambdas into the space.  O(N k) data never leaves its rank
 * except as the edges themselves. */
as_status as_graph_shard_csr(as_space* sp, const as_graph_params* gp, int64_t n_global, int64_t row_offset,
                             const int32_t* idx_dev, const double* dist_dev, const double* gy_dev, const int32_t* cnt_dev,
                             int64_t n_in, const int32_t* in_row_dev, const int32_t* in_col_dev, const double* in_dist_dev,
                             const double* in_gy_dev, as_graph** out_graph);
as_status as_graph_deg_copy(const as_graph* gr, double* out_dev);
as_status as_graph_shard_energy(as_space* sp, as_graph* gr, const double* deg_global_dev, const double* n64_global_dev);
as_status as_graph_energy_copy(const as_graph* gr, double* out_dev);
as_status as_graph_shard_lambdas(as_space* sp, as_graph* gr, const double* E_global_dev, int64_t n_global);
int64_t as_graph_row_offset(const as_graph* gr);      /* first row a sharded graph holds (0 for a whole graph) */
int64_t as_graph_ncols(const as_graph* gr);           /* items the graph's columns range over */
int64_t as_graph_nitems(const as_graph* gr);         /* items the whole index covers (all ranks' rows), item or feature mode */

/* ---- staged build, feature mode (AS_LAMBDA_FEATURE): what as_build composes when opts->lambda_mode selects
 *      the F x F feature-space Laplacian; multi-GPU hosts call the steps with a row range per rank and exchange
 *      the D x D Gram partials and the N energies in between ---- */

/* step 2f: Gram of the columns over items [row_begin, row_end): out_gram_dev[a*d + b] = sum_i x_ia x_ib
 * (fp64, d x d, symmetric, device).  Partial Grams of disjoint row ranges add up to the full one. */
as_status as_feat_gram(const as_space* sp, int64_t row_begin, int64_t row_end, double* out_gram_dev);
/* step 3f: feature graph (k-NN over the D columns, union symmetrisation, weights, degrees; L = D - W) from
 * the complete Gram. */
as_status as_feat_graph(const as_space* sp, const as_graph_params* gp, const double* gram_dev, as_graph** out_graph);
/* step 4f: Rayleigh energy E and dispersion G of items [row_begin, row_end), written at those positions of
 * the n-long device arrays. */
as_status as_feat_energy(const as_space* sp, const as_graph* gr, int64_t row_begin, int64_t row_end,
                         double* E_dev, double* G_dev);
/* step 5f: tau0 = median of the positive E, lambdas of all n items into the space (E, G complete, device). */
as_status as_feat_lambdas(as_space* sp, as_graph* gr, const double* E_dev, const double* G_dev);
/* row-sharded form: E, G of ALL n_global items; this shard (rows [row_offset, row_offset + nitems)) gets its lambdas */
as_status as_feat_lambdas_global(as_space* sp, as_graph* gr, const double* E_dev, const double* G_dev, int64_t n_global,
                                 int64_t row_offset);

/* ---- search: replaces prepare_query_item + search_lambda_aware, src/lib.rs:154,173 ---- */

/* query: host fp64, contiguous, length d (d != nfeatures -> AS_EINVAL,
 * src/lib.rs:140-146).  out_idx/out_score: capacity >= min(topk, nitems).
 * lambda_q == 0 -> AS_EZEROLAMBDA.  Results: score desc, index asc.
 * RE-ENTRANT across host threads: every call runs on a workspace of its own -- stream, device buffers, pinned
 * results -- taken from a pool the space grows on demand (up to 4, ARROWSPACE_SEARCH_POOL); no lock is held while a
 * search runs, so one thread's scan overlaps another's finish kernel and host turnaround.  The reference holds the GIL
 * through prepare_query_item + search_lambda_aware (src/lib.rs:132-174): its searches are serialised. */
as_status as_search(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau,
                    int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q);
/* matrix pipe the last k-NN pass over this space's rows ran on (as_build, as_knn_rows): 0 fp32 (ARROWSPACE_K2_FP32=1), 1 bf16
 * head + tail, 2 int8 two-digit image (the default where the items' quantisation error allows it); -1: none yet.  The graphs
 * are the same bits on every pipe: the pipe only prefilters, the refinement is exact. */
int32_t as_space_knn_pipe(const as_space* sp);
/* 1 when the last single-query scan (of this workspace / of the space's first pooled workspace) read the int8 two-digit image
 * of the items -- half the bytes of the fp32 matrix -- instead of the fp32 matrix (ARROWSPACE_SCAN_FP32=1, rows wider than 2 048
 * floats, queries or items the image represents badly).  Either way the scan only prefilters: results are exact. */
int32_t as_query_scan_int8(const as_query* q);
int32_t as_last_scan_int8(const as_space* sp);
/* Width in bits of the coarse operand that scan read: 4 when it took the NIBBLE tiles (the items quantised afresh to 16 levels per
 * row, half the bytes of the high digits), 8 otherwise -- as_query_scan_int8 keeps answering 2 for the coarse scan at
 * either width.  as_set_tuning("coarse_bits", v) / ARROWSPACE_COARSE_BITS: -1 the library decides (default), 8 never the nibble
 * tiles, 4 the nibble tiles wherever rows of 512 columns and more allow them, at any row count. */
int32_t as_query_scan_bits(const as_query* q);
int32_t as_last_scan_bits(const as_space* sp);
/* Debugging aid (tests of the nibble tiles).  as_debug_nibble_image makes the image if need be and reports info[0] = 1 when it is
 * usable (0: a zero or non-finite row, rows outside 512 .. 4 096 columns, no memory), info[1] = R4 = max_i |x_i - x~_i| / |x_i|,
 * info[2] = 32-column chunks per row, info[3] = rows of the image; tiles (may be null; info[3] * info[2] * 16 bytes,
 * [tile][chunk][64 rows][16 bytes]) and fa4 (may be null; nrows level steps) are copied to the host. */
as_status as_debug_nibble_image(const as_space* sp, void* tiles, int64_t tiles_bytes, float* fa4, int64_t nrows, double* info);
/* Debugging aid (tests of the int8 two-digit image).  as_debug_i8_image makes the image if need be and reports in info[0..6]: 1 when
 * it is there and usable (0: a non-finite item, no memory), U = max_i s_i |theta_i|_2 / (16256 |x_i|), V = max_i s_i |a2_i|_2 /
 * (16256 |x_i|), the coefficient 2.001 U + V^2 + 12 * 2^-24 (beyond 1e-3 the k-NN block takes the bf16 pipe), dp8 (the columns
 * rounded up to 64), the rows of the image (items padded to the row tile, plus one tile), the bad flag (1 non-finite item, 2 no
 * memory).  Copied to the host, each only where its pointer is not null: x8 (rows * dp8 * 2 bytes: per row and 64-column slab 64
 * bytes of high digits a1, then 64 of low digits a2), fa8 (nrows scales s_i sqrt(128) / 16256) and x8h (rows * dp8 bytes: the high
 * digits alone as the coarse scan reads them, [tile of 64 rows][16-column chunk][64 rows][16 bytes]; made if need be). */
as_status as_debug_i8_image(const as_space* sp, void* x8, int64_t x8_bytes, float* fa8, int64_t nrows, void* x8h, int64_t x8h_bytes, double* info);
/* 1 when the last batched pass of as_search_batch (its first workspace) ran on the int8 images of items and queries
 * (v_mfma_i32_32x32x32_i8, three products per column) rather than on the bf16 head + tail of the fp32 items. */
int32_t as_last_batch_int8(const as_space* sp);
/* Scans of as_search_batch that served TWO passes (64 queries) with one read of the items: calls of more than 32 queries launch
 * their passes in pairs, and a pair on the int8 images of rows up to 768 columns shares its scan (ARROWSPACE_NO_BATCH_DUAL=1:
 * never).  A count since the space was made. */
int64_t as_batch_dual_scans(const as_space* sp);
/* workspaces the pool of as_search holds at the moment (1 after single-threaded use) */
int32_t as_search_pool_size(const as_space* sp);
/* Concurrent as_search callers on one space share a pass over the items where they can (coarse scans of tau >= 0.4 searches that
 * arrive within a few microseconds of each other run as ONE launch for up to four queries: "gang scans"; ARROWSPACE_GANG=0:
 * never).  out[i] = scans this space launched through that path with i + 1 members (i = 0 .. 3); out[4 .. 9] = host-prepared scans
 * that did not take it, by first reason: no concurrent callers lately, not a search for the fused tail (tau < 0.4, crowded
 * candidates lately), not a coarse scan, per-search state still to be reset, per-launch timing on, a row range.  Results never
 * depend on any of it. */
as_status as_gang_counters(const as_space* sp, int64_t* out, int32_t n);

/* B queries, row-major [b][d]; outputs [b][topk]; status per query in out_status
 * (AS_OK / AS_EZEROLAMBDA).  Extension. */
as_status as_search_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d,
                          double tau, int64_t* out_idx, double* out_score, int64_t* out_len,
                          double* out_lambda_q, int32_t* out_status);

/* ---- staged search (row-sharded multi-GPU; as_search composes these on one GPU) ---- */

/* fixed-size device records exchanged between ranks.
 * THE TWO MERGES (as_query_lambda / _batch over as_knn_rec, as_query_finish / _batch over as_hit_rec; both run identically on
 * every rank over the all-gathered records; tests/test_gpu_staged_records.py states all of it against oracle/oracle_np.py):
 *   - an EMPTY slot is idx == -1, anywhere in the buffer; none of its other fields is ever read, whatever they hold;
 *   - k-NN records are ordered by (key ascending, idx ascending) and the first k valid ones are the query's neighbours: lambda_q
 *     comes from their dist / gy / deg / ny alone, summed in that order (the same bits whatever the layout of the records);
 *     hit records by (score descending, idx ascending; +0.0 and -0.0 tie), cut at topk; a valid hit may carry -inf;
 *   - at most as_record_capacity(0) = 1 024 k-NN records (ranks x k) and as_record_capacity(1) = 8 208 hit records
 *     (ranks x (topk + 1)) per query; one more returns AS_EUNSUPPORTED and nothing is launched: the workspace keeps the state of
 *     the previous step;
 *   - a hit record with idx == -2 is a FLAG record: (int)score holds bits, OR-ed over all such records of the merge (none at
 *     all = 0) and with the flags of the workspace's own scan.  1: the k-NN list is not provably exact, 2: nor the scorer's
 *     (as_query_flags bit 0 of knn_inexact / score_inexact), 4: the k-NN candidate buffer overflowed, 8: the scorer's (bit 1
 *     of the same), 16: a rank's candidates did not fit its one-exchange block (as_query_x1_redo), 32: a rank failed its part
 *     of as_query_search_staged -- neither of the last two shows in as_query_flags.  The batched finish reports a slot with any
 *     bit as out_status -1, out_len 0;
 *   - NO id may occur twice among the valid records of one merge (the ranks own disjoint rows): two equal (key, idx) or
 *     (score, idx) pairs would take the same rank and leave the place behind it unwritten.  Ids are below 2^31 - 1;
 *   - m == 0 (any non-null pointer), only empty slots, weights that all underflow or edge energies that are all zero give
 *     lambda_q == 0: the following finish returns AS_EZEROLAMBDA, out_len 0, whatever hit records it is handed;
 *   - under AS_LAMBDA_FEATURE as_query_lambda / _batch are no-ops behind their checks: lambda_q is the scan's;
 *   - per as_query_scan: as_query_lambda and as_query_finish may be repeated, as_query_score runs ONCE (the scorer appends
 *     its candidates behind the previous call's until a scan resets the count). */
typedef struct {
    int64_t idx;  /* global item index, -1 = empty slot */
    double key;   /* eps-test / ordering key: squared L2 distance or cosine distance */
    double dist;  /* d(q, x_idx) */
    double gy;    /* y_q . y_idx */
    double deg;   /* degree of item idx in the index graph */
    double ny;    /* |y_idx|^2 */
} as_knn_rec;

typedef struct {
    int64_t idx; /* global item index, -1 = empty slot */
    double score;
} as_hit_rec;

as_status as_query_create(const as_space* sp, const as_graph* gr, as_query** out);
void as_query_free(as_query* q);
/* rows [row_begin,row_end) are this rank's shard; row_offset maps local rows of a
 * shard-only space to global indices (0 when the space holds all items). */
as_status as_query_scan(as_query* q, const double* query_host, int64_t d, int64_t row_begin, int64_t row_end);
/* k records: this shard's exact nearest items to the query (device pointer) */
const as_knn_rec* as_query_knn_records(const as_query* q);
int64_t as_query_knn_capacity(const as_query* q);
/* lambda_q from m records (own, or all-gathered from every rank) */
as_status as_query_lambda(as_query* q, const as_knn_rec* recs_dev, int64_t m);
/* local scoring of the scanned rows; topk records */
as_status as_query_score(as_query* q, double tau);
const as_hit_rec* as_query_hit_records(const as_query* q);
int64_t as_query_hit_capacity(const as_query* q);
/* merge m hit records (own or all-gathered), copy to host; synchronises. */
as_status as_query_finish(as_query* q, const as_hit_rec* hits_dev, int64_t m, int64_t* out_idx,
                          double* out_score, int64_t* out_len, double* out_lambda_q);
/* Batched staged search (extension: 32 query slots per pass over this rank's rows, GEMM-shaped scan; the two
 * record exchanges of a pass are amortised over the slots).  Record buffers: [slot][k] as_knn_rec and
 * [slot][topk + 1] as_hit_rec (as_query_bind_records); the all-gathered buffers handed back are
 * [rank][slot][...].  out_status[b]: AS_OK / AS_EZEROLAMBDA, or -1 = rerun query b through the single-query steps. */
as_status as_query_create_batch(const as_space* sp, const as_graph* gr, as_query** out);
int32_t as_query_slots(const as_query* q);
as_status as_query_scan_batch(as_query* q, const double* queries_host, int32_t nb, int64_t d, int64_t row_begin, int64_t row_end);
as_status as_query_lambda_batch(as_query* q, const as_knn_rec* recs_dev, int32_t nranks);
as_status as_query_score_batch(as_query* q, double tau);
as_status as_query_finish_batch(as_query* q, const as_hit_rec* hits_dev, int32_t nranks, int64_t* out_idx, double* out_score,
                                int64_t* out_len, double* out_lambda_q, int32_t* out_status);
/* flags bit0: run the following scans in fp64 end to end (the fallback as_search takes when
 * the fp32 candidate lists are not provably exact); bit1: wavefront-list selection instead
 * of the filter buffers (taken when a buffer overflowed); bit2: the next as_query_scan does
 * not scan -- it re-derives the k-NN candidates of the SAME query and row range from the dot
 * products the previous scan left in HBM (threshold selection; taken when only the k-NN
 * buffer overflowed: more than 4096 rows inside eps).  as_query_flags reports the last
 * finished search: bit0 = not provably exact, bit1 = this side's candidate buffer overflowed
 * (knn_inexact: the k-NN buffer, score_inexact: the scorer's). */
void as_query_set_exact(as_query* q, int32_t flags);
as_status as_query_flags(const as_query* q, int32_t* knn_inexact, int32_t* score_inexact);
/* ONE exchange per sharded query (tau in [0.4, 1], item-graph lambda; as_query_x1_usable says so, identically on every rank):
 * as_query_x1_begin scans this rank's rows and finishes what only this rank can finish -- its k exact nearest rows (records)
 * and the exact cosine and lambda of every row its scan kept as a scorer candidate -- into ONE block of as_query_x1_bytes
 * bytes at send_dev (device memory of the caller: an all-gather send buffer); the host all-gathers the blocks of the `world`
 * ranks in rank order; as_query_x1_finish forms lambda_q, scores and ranks every rank's candidates (identically on every rank)
 * and copies the answer out.  Afterwards as_query_flags as after as_query_finish; as_query_x1_redo != 0: some rank's candidates
 * did not fit its block (or it had none to offer): run the query again through as_query_scan / _lambda / _score / _finish.
 * as_query_search_staged takes this pass by itself (ARROWSPACE_STAGED_X1=0: never).
 * Serves PyArrowSpace::search, /root/reference/src/lib.rs:132-174, on a row-sharded index. */
int64_t as_query_x1_bytes(const as_query* q, int32_t world);
int32_t as_query_x1_usable(const as_query* q, double tau);
/* The pass's switch is a property of the workspace: read from ARROWSPACE_STAGED_X1 when the workspace is made
 * (as_query_x1_enabled), set for good by as_query_set_x1 -- the host of a row-sharded index agrees on it over its ranks (one
 * all-reduce, MIN) when it opens the query: every rank must issue the same collectives for every query that follows. */
int32_t as_query_x1_enabled(const as_query* q);
void as_query_set_x1(as_query* q, int32_t enabled);
as_status as_query_x1_begin(as_query* q, const double* query_host, int64_t d, int64_t row_begin, int64_t row_end, double tau, void* send_dev,
                            int32_t world);
as_status as_query_x1_finish(as_query* q, const void* all_dev, int32_t world, double tau, int64_t* out_idx, double* out_score, int64_t* out_len,
                             double* out_lambda_q);
int32_t as_query_x1_redo(const as_query* q);
/* A pass that came back with as_query_x1_redo != 0 may be the coarse scan's doing (tau >= 0.4: a rank scans the high digits of
 * its int8 image alone, with wider candidate windows): as_query_set_coarse(q, 0), run the pass once more (every rank alike),
 * as_query_set_coarse(q, 1); only if it comes back with redo again take the two-exchange steps. */
void as_query_set_coarse(as_query* q, int32_t allowed);
int64_t as_query_x1_passes(const as_query* q);   /* one-exchange passes this workspace has finished */
/* The per-query exchange steps issued by the library itself (RCCL on the query's stream; librccl is taken from the
 * process or /opt/rocm/lib by dlopen -- as_comm_available() == 0 on a box without it).  The ranks of an index share one
 * communicator: rank 0 draws an id (as_comm_unique_id: 128 bytes), the host hands it to every rank (any broadcast),
 * every rank calls as_comm_create (collective).  as_query_set_comm binds a single-query workspace to it;
 * as_query_search_staged is then ONE host call per query: the one-exchange pass above where it applies, else scan of this
 * rank's rows, all-gather of the k-NN records, lambda_q, scorer, all-gather of the hit records, merge; and the escalation to
 * the exact paths (every rank with the same query and tau; same results and errors as as_search on one space holding
 * every item).
 * Serves PyArrowSpace::search, /root/reference/src/lib.rs:132-174, on a row-sharded index. */
typedef struct as_comm as_comm;
int32_t as_comm_available(void);
as_status as_comm_unique_id(void* out_128_bytes);
as_status as_comm_create(const void* id_128_bytes, int32_t rank, int32_t world, int32_t device, as_comm** out);
void as_comm_free(as_comm* c);
as_status as_query_set_comm(as_query* q, as_comm* c);
as_status as_query_search_staged(as_query* q, const double* query_host, int64_t d, int64_t row_begin, int64_t row_end, double tau,
                                 int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q);
/* HIP stream (hipStream_t) the query's kernels run on, for event timing / ordering;
 * as_query_set_stream makes them run on the caller's stream (NULL restores the private one),
 * e.g. the stream torch.distributed orders its RCCL collectives against. */
void as_query_set_stream(as_query* q, void* hip_stream);
/* Make the query write its k k-NN records and its topk+1 hit records (the last one carries
 * the exactness flags) into caller-owned device buffers, e.g. all-gather send buffers. */
as_status as_query_bind_records(as_query* q, as_knn_rec* knn_dev, as_hit_rec* hits_dev);
void* as_query_stream(const as_query* q);

/* ---- accessors: src/lib.rs:40-61 (GraphLaplacian), 78-124 (ArrowSpace) ---- */
/* searches on this space whose answer was returned although it failed its a-posteriori check even on the strongest
 * (fp64) path: more near-ties at the k-th distance / score than fp64 can order.  0 in normal operation. */
int64_t as_unproven_searches(const as_space* sp);
int64_t as_nitems(const as_space* sp);
int64_t as_nfeatures(const as_space* sp);
as_status as_get_item(const as_space* sp, int64_t idx, double* out_vec, double* out_lambda);
as_status as_lambdas(const as_space* sp, double* out);
int64_t as_nnodes(const as_graph* gr);
as_status as_get_graph_params(const as_graph* gr, as_graph_params* out); /* sigma resolved */
int64_t as_graph_nnz(const as_graph* gr); /* stored Laplacian entries incl. diagonal */
/* CSR of the normalised Laplacian: indptr int64[n+1], indices int64[nnz], values fp64[nnz] */
as_status as_graph_csr(const as_graph* gr, int64_t* indptr, int64_t* indices, double* values);
/* the stored CSR of an item graph as the device holds it, without the diagonal: indptr int64[n+1], indices int64[indptr[n]],
 * dist fp64[indptr[n]] the distance d_ij of every entry (as_graph_nnz minus n entries at most); a feature-mode graph stores no
 * distances (AS_EUNSUPPORTED) */
as_status as_graph_csr_dist(const as_graph* gr, int64_t* indptr, int64_t* indices, double* dist);
as_status as_graph_degrees(const as_graph* gr, double* out);
double as_graph_tau0(const as_graph* gr);
int32_t as_graph_lambda_mode(const as_graph* gr); /* AS_LAMBDA_* */
/* device pointer to the fp64 lambdas (n) -- for multi-GPU hosts */
const double* as_lambdas_dev(const as_space* sp);

/* per-stage seconds of the last build, and kernel-only seconds of the X.X^T block:
 * out[0]=ingest out[1]=knn_mfma out[2]=refine out[3]=fallback_exact out[4]=graph
 * out[5]=total out[6]=fallback_rows (rows recomputed by the row-serial fp64 path) out[7]=mfma_flops_issued
 * out[8]=unproven_rows (fallback rows whose list could still not be proven exact: more near-ties at the k-th
 * distance than the widest candidate list holds, inside fp64 rounding of one another) out[9]=band_rows (rows
 * settled by the second, band-collecting pass) */
as_status as_build_stats(const as_graph* gr, double* out, int32_t n);
/* per-stage device microseconds of the last search on q (HIP events):
 * out[0]=scan out[1]=rest out[2]=exact_fallback_used */
as_status as_query_stats(const as_query* q, double* out, int32_t n);

/* HIP-event timing of searches is off by default (the events cost a few microseconds per
 * query); enable it before the searches whose stats are read */
void as_enable_search_stats(int32_t enabled);
/* Measurement knob, no reference counterpart: launch parameters the library otherwise picks itself.  "tile_geom" = <blocks per
 * CU><two digits: ring KiB per wave> of the single query's tile scan (e.g. 406, 308, 216; ARROWSPACE_TILE_GEOM at load);
 * "x1_blocks" = blocks of the coarse scan's exact-evaluation kernel (16 .. 256, default 128).
 * "coarse_bits" = -1 / 8 / 4: width of the single query's coarse operand (as_query_scan_bits).
 * "x1_final_rank" = 1 / 0: the fused tail's final kernel / its first kernel's last block ranks the rows inside eps, for every
 * workspace; any other value: each workspace's own switch again (ARROWSPACE_X1_FINAL_RANK when it was made; default 1).
 * "subset_batch_mib" = MiB of scores one chunk of queries of the batched filtered forms may hold (default 256; <= 0: the default);
 * the per-query list forms chunk by it too.  "lists_timing" = 1 / 0: HIP events around their score kernel (as_lists_kernel_us).
 * "range_cap" = entries of the append buffer a range call starts with (default 65 536, or what earlier overflows grew the buffer
 * to; <= 0: the default); "range_timing" = 1 / 0: HIP events around the range forms' compaction kernel (as_range_kernel_us).
 * "diverse_chunk" = queries per launch of the diversified forms (default 4096; <= 0: the default); "diverse_timing" = 1 / 0: HIP
 * events around their select kernel (as_diverse_kernel_us).  "fused_timing" = 1 / 0: HIP events around the fused forms'
 * accumulate kernel (as_fused_kernel_us).  "grouped_timing" = 1 / 0: HIP events around the grouped forms' pick kernels
 * (as_grouped_kernel_us).  "maxsim_timing" = 1 / 0: HIP events around late-interaction search's pass A and fold kernel
 * (as_maxsim_kernel_us).  "fused_batch_timing" = 1 / 0: HIP events around the batched fused forms' accumulate kernel
 * (as_fused_batch_kernel_us); "fused_batch_mib" = MiB of accumulator rows one group of needs of those forms may hold (default
 * 256; 0: the default; v < 0: -v KiB, so that tests reach several groups at small shapes).  "maxsim_batch_timing" = 1 / 0: HIP
 * events around batched late-interaction search's pass A and segmented fold kernel (as_maxsim_batch_kernel_us);
 * "maxsim_batch_mib" = MiB of accumulator rows one group of needs of those forms may hold (same values as "fused_batch_mib").
 * "maxsim_lists_timing" = 1 / 0: HIP events around the score kernel, the fold kernel and the selection of late-interaction
 * re-ranking of per-need documents (as_maxsim_lists_kernel_us); those forms chunk by "subset_batch_mib" too.
 * "filtered_grid_cap" = v > 0: gridDim.x of the filtered family's stride-loop kernels (the gather score
 * kernels of the subset and list forms, the radix select's passes, the fused and late-interaction folds, the grouped picks, the range compaction) is
 * clipped to at most v blocks, so tests reach the later trips of those loops at small shapes; 0 (default): no clip.
 * Returns 0, or 1 for an unknown key.  Results never depend on it. */
int32_t as_set_tuning(const char* key, int32_t value);
/* same, for the workspace as_search keeps inside the space (last as_search call) */
as_status as_last_search_stats(const as_space* sp, double* out, int32_t n);
/* single-query searches on this space since it was made: out[0] searches, [1] zero-lambda results (src/lib.rs:156-159),
 * [2] reruns after a failed k-NN a-posteriori check, [3] after a candidate-buffer overflow, [4] after a failed scorer
 * check, [5] searches that took at least one rerun.  A rerun costs a second pass over the items.  [6] scans that read the nibble
 * tiles, [7] those of them whose search was redone on the 8-bit tiles (not counted in [2] .. [5]). */
as_status as_search_counters(const as_space* sp, int64_t* out, int32_t n);
/* Extension: one query under ntau taus (a tau sweep) -- list j, at out_idx / out_score + j * topk' (topk' = min(topk, nitems)),
 * out_len[j] entries, is what as_search returns for taus[j].  lambda_q (one value, tau-independent) -> out_lambda_q; lambda_q == 0
 * -> AS_EZEROLAMBDA.  Taus in [0, 1] share passes over the items, up to 8 per pass: one coarse scan, k-NN records and lambda_q,
 * the union of the taus' candidate sets evaluated exactly once, one ranking per tau.  Equal taus are computed once; a tau outside
 * [0, 1] (or NaN), a sweep of one distinct tau, and whatever a shared pass does not serve take the single search.  ntau = 0:
 * nothing is launched.  Re-entrant as as_search (one workspace of the pool per call). */
as_status as_search_taus(const as_space* sp, const as_graph* gr, const double* query, int64_t d, const double* taus, int64_t ntau,
                         int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q);
/* out[0] as_search_taus calls, [1] shared passes that served at least one tau, [2] taus a shared pass did not serve, or could not
 * be run for (feature graphs, force_exact, a scan the image cannot serve, ...), redone by the single search */
as_status as_sweep_counters(const as_space* sp, int64_t* out, int32_t n);
/* Extension: b queries (row-major [b][d]) under ntau taus -- list (i, j), at out_idx / out_score + (i * ntau + j) * topk'
 * (topk' = min(topk, nitems)), out_len[i * ntau + j] entries, is what as_search returns for query i and taus[j].  lambda_q per
 * query -> out_lambda_q[i]; out_status[i] AS_OK / AS_EZEROLAMBDA (lambda_q == 0: every list of that query is empty).  Where
 * as_search_batch batches (b > 1, no force_exact or search mode, no feature lambdas) the distinct taus in [0, 1] share batched
 * passes, up to 8 per pass: one scan, k-NN step and lambda_q per 32 queries, a scorer tail per (query, tau) pair.  Equal taus are
 * computed once; every other tau takes as_search_batch's route, and whatever a shared pass does not serve the single search.
 * Serialised with as_search_batch (the batched workspaces). */
as_status as_search_batch_taus(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d,
                               const double* taus, int64_t ntau, int64_t* out_idx, double* out_score, int64_t* out_len,
                               double* out_lambda_q, int32_t* out_status);
/* out[0] as_search_batch_taus calls, [1] batched passes whose scorer tail served a tau sweep, [2] (query, tau) pairs those passes
 * served, [3] pairs they left to the single search */
as_status as_batch_sweep_counters(const as_space* sp, int64_t* out, int32_t n);

/* ---- Extension: filtered search.  A subset restricts which items a search may return; it does not change the index: lambda_q is
 * the query's lambda against the whole index, the items' lambdas are their own -- the values as_search uses.
 * as_subset_create: m item ids in HOST memory, any order, duplicates allowed (m = 0: the empty set); they are sorted and made
 * unique once, on the host, and kept in device memory together with every buffer a search over them needs (scores, the
 * selection's histograms, the pinned result): nothing is allocated per query.  An id outside [0, nitems) -> AS_EINVAL.  The
 * handle belongs to the space it was made for (any other space -> AS_EINVAL) and must be freed before it. */
typedef struct as_subset as_subset;
as_status as_subset_create(const as_space* sp, const int64_t* ids_host, int64_t m, as_subset** out);
int64_t as_subset_size(const as_subset* sub);                 /* distinct ids; 0 for NULL */
as_status as_subset_ids(const as_subset* sub, int64_t* out);  /* sorted, unique: as_subset_size entries */
void as_subset_free(as_subset* sub);                          /* NULL: no-op */
/* The first min(topk, |S|) items of the subset by (S11 score descending, index ascending): with every item in S, what as_search
 * returns.  Cost: ONE ORDINARY as_search per call (lambda_q comes from it, hits discarded: the same escalation, the same
 * AS_EZEROLAMBDA -- whatever S is, the empty set included -- and the same out_lambda_q), then a gather of the subset's rows
 * (fp64 items where the space keeps them, else fp32 widened; fp64 dot, the exact score of as_search) and an exact selection on
 * the device.  Wrong d -> AS_EINVAL ("query length ... must match nfeatures ..."), non-finite tau -> AS_EINVAL, a shard of a
 * row-sharded index -> AS_EUNSUPPORTED.  Calls on one handle are serialised; different handles and as_search run beside it. */
as_status as_search_subset(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, const as_subset* sub,
                           int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q);
/* out_scores[i] = the S11 score of item ids_host[i] (the caller's order, duplicates kept): the same kernel without the selection,
 * the same checks and the same one as_search per call.  Its device buffers live in the space and grow on demand; calls on one
 * space are serialised. */
as_status as_score_items(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, const int64_t* ids_host,
                         int64_t m, double* out_scores, double* out_lambda_q);
/* measurement: HIP events around the score kernel of as_search_subset on this handle (off by default), and the device
 * microseconds of the last timed call */
void as_subset_set_timing(as_subset* sub, int32_t enabled);
double as_subset_kernel_us(const as_subset* sub);
/* The batched forms: b queries, row-major [b][d] in HOST memory, against one subset / one id list.  List i (out_idx / out_score +
 * i * kk, kk = min(topk, nitems, |S|), out_len[i] entries) is what as_search_subset returns for query i; out_scores [b][m] row i is
 * what as_score_items returns for it.  The summation order differs from the single forms' (an fp64 GEMM on the matrix cores, one
 * accumulation chain over the columns per score): scores agree to 1e-12 relative, indices except inside such ties; identical
 * rows still score bit-equal and come back in index order.  lambda_q and out_status[i] (AS_OK or AS_EZEROLAMBDA: that query gets
 * out_len 0, its row of out_scores is left unwritten) come from ONE as_search_batch call over all b queries, hits discarded.
 * Checks and messages are the single forms'; b == 0 launches nothing; an empty subset / m == 0 still runs the lambda_q step.
 * The gathered rows are read once per tile of 64 queries; queries run in chunks whose scores fit a budget (256 MiB;
 * as_set_tuning("subset_batch_mib")), one stream wait per chunk.  The batched buffers are made on the first batched call on a
 * handle (as_score_items_batch: in the space) and grow on demand.  out_lambda_q and out_status may be NULL.  With timing enabled
 * as_subset_kernel_us reports the batched score kernel summed over the chunks of the last call. */
as_status as_search_subset_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                 const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q,
                                 int32_t* out_status);
as_status as_score_items_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                               const int64_t* ids_host, int64_t m, double* out_scores, double* out_lambda_q, int32_t* out_status);
/* Tau sweeps over a subset: the four filtered forms under ntau taus, with ONE lambda_q step (lambda_q does not depend on tau: the
 * single search, or ONE as_search_batch call, run with taus[0], hits discarded) and ONE gather of the subset's rows per up to 8
 * distinct taus: every (query, item) cosine is formed once and blended with each tau of the group.  Layouts as as_search_taus /
 * as_search_batch_taus: list (i, j) at out_idx / out_score + (i * ntau + j) * kk, kk = min(topk, nitems, |S|), out_len[i * ntau + j]
 * entries (the single forms: i = 0); out_scores [ntau][m], batched [b][ntau][m]; one out_lambda_q per query, one out_status per
 * query of the batched forms.  List j / row j is what the single-tau form of the same route returns for taus[j]: the same score
 * bits given the same lambda_q (as_search_subset / as_score_items for the single forms, as_search_subset_batch /
 * as_score_items_batch for the batched ones); across routes 1e-12 relative as documented above.  Every finite tau is served; a
 * NaN or infinite tau anywhere in the list -> AS_EINVAL before anything is launched.  Taus equal by bit pattern are computed
 * once, their lists / rows copied.  ntau == 0 launches nothing.  The other checks, codes and messages are the single-tau forms';
 * lambda_q == 0 -> AS_EZEROLAMBDA (batched: out_status, out_len 0 for every list of that query, its rows of out_scores left
 * unwritten), whatever the subset; an empty subset / m == 0 still runs the lambda_q step.  The batched forms pick the taus per
 * gather (<= 8) and the queries per chunk from the "subset_batch_mib" budget; results never depend on either.  The sweep's
 * buffers are made on a handle's first sweep (as_score_items*_taus: in the space) and grow on demand.  Serialised as the
 * single-tau forms.  With timing enabled as_subset_kernel_us reports the sweep's score kernel summed over the call's launches. */
as_status as_search_subset_taus(const as_space* sp, const as_graph* gr, const double* query, int64_t d, const double* taus, int64_t ntau,
                                const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q);
as_status as_score_items_taus(const as_space* sp, const as_graph* gr, const double* query, int64_t d, const double* taus, int64_t ntau,
                              const int64_t* ids_host, int64_t m, double* out_scores, double* out_lambda_q);
as_status as_search_subset_batch_taus(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d,
                                      const double* taus, int64_t ntau, const as_subset* sub, int64_t* out_idx, double* out_score,
                                      int64_t* out_len, double* out_lambda_q, int32_t* out_status);
as_status as_score_items_batch_taus(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d,
                                    const double* taus, int64_t ntau, const int64_t* ids_host, int64_t m, double* out_scores,
                                    double* out_lambda_q, int32_t* out_status);
/* out[0] tau sweeps over a subset (the four calls above), [1] score-kernel launches they made, [2] tau planes those launches wrote,
 * [3] lambda_q steps run (single searches plus as_search_batch calls) */
as_status as_subset_sweep_counters(const as_space* sp, int64_t* out, int32_t n);
/* Per-query candidate lists (re-ranking): b queries, row-major [b][d] in HOST memory, EACH WITH ITS OWN id list -- list i is
 * ids_host[offsets_host[i] .. offsets_host[i + 1]) (offsets_host: b + 1 entries, offsets[0] == 0, non-decreasing; any order,
 * duplicates allowed, lists may be empty and may share ids).  as_score_lists_batch: out_scores[offsets[i] + j] = what
 * as_score_items returns for query i and entry j of its list (the caller's order, duplicates kept).  as_search_lists_batch: list
 * i, at out_idx / out_score + i * kk (kk = min(topk, nitems)), out_len[i] = min(kk, distinct ids of list i) entries, is what
 * as_search_subset returns for query i over its list.  Scores agree with the single forms to 1e-12 relative, indices except inside
 * such ties.  The bits of the score of (query i, item j) depend on that query, that row, tau and lambda_q only -- not on the
 * entry's position, the other lists of the call, the chunk budget or which of the two forms ran: identical rows score bit-equal
 * and come back in index order, an id listed twice gets the same bits twice.  lambda_q and out_status[i] (AS_OK or
 * AS_EZEROLAMBDA: that query gets out_len 0, its scores are left unwritten, the others are served) come from ONE as_search_batch
 * call over all b queries, hits discarded; empty lists still run it; b == 0 launches nothing.  Checked before anything is
 * launched, that step included: a null argument ("<name>: null argument", nothing written), offsets that do not start at 0 or
 * decrease, an id outside [0, nitems) (the message names the id and its list) -> AS_EINVAL; offsets[b] >= 2^31 -> AS_EUNSUPPORTED;
 * wrong d, a non-finite tau and a shard of a row-sharded index as the single forms.  out_lambda_q and out_status may be NULL.
 * One ragged launch scores all pairs of a chunk of queries (the lists cut into segments of at most 64 entries, a block per segment, the
 * single form's summation order per row), one block per list selects (the search form removes each list's repeated ids on the
 * host first); queries run in chunks whose scores fit the "subset_batch_mib" budget, a list longer than it a chunk of its own,
 * one stream wait per chunk.  The buffers live in the space and grow on demand; calls on one space are serialised, as_search runs
 * beside them. */
as_status as_score_lists_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                               const int64_t* ids_host, const int64_t* offsets_host, double* out_scores, double* out_lambda_q,
                               int32_t* out_status);
as_status as_search_lists_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                const int64_t* ids_host, const int64_t* offsets_host, int64_t* out_idx, double* out_score,
                                int64_t* out_len, double* out_lambda_q, int32_t* out_status);
/* out[0] calls of the two entries above that passed their checks, [1] score-kernel launches they made, [2] (query, item) pairs
 * those launches scored, [3] lambda_q steps run (as_search_batch calls), [4] host nanoseconds spent on id checks, deduplication and
 * work tables */
as_status as_lists_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement: the device microseconds of the ragged score kernel, summed over the chunks of the last call on this space that
 * ran under as_set_tuning("lists_timing", 1) (HIP events around the kernel; off by default) */
double as_lists_kernel_us(const as_space* sp);
/* Tau sweeps over per-query candidate lists: the two forms above under ntau taus, with ONE lambda_q step (ONE as_search_batch call
 * over all b queries, run with taus[0], hits discarded), ONE upload per chunk of queries and ONE ragged gather per chunk and up to
 * 8 distinct taus: every (query, item) cosine is formed once and blended with each tau of the group.  Query-major layouts.
 * as_score_lists_batch_taus: with m_i = offsets[i + 1] - offsets[i], the score of (query i, tau j, entry e) is at
 * out_scores[ntau * offsets[i] + j * m_i + e]: query i owns one contiguous [ntau][m_i] block, row j of it is what
 * as_score_lists_batch writes for query i under taus[j] (the caller's order, duplicates kept).  as_search_lists_batch_taus: list
 * (i, j) at out_idx / out_score + (i * ntau + j) * kk, kk = min(topk, nitems), out_len[i * ntau + j] = min(kk, distinct ids of list
 * i) entries, is what as_search_lists_batch returns for query i under taus[j].  The same score bits as the single-tau forms given
 * the same lambda_q; the two sweep forms give the same bits for the same (query, tau, item).  One out_lambda_q and one out_status
 * per query (both may be NULL); lambda_q == 0 -> AS_EZEROLAMBDA in out_status, out_len 0 for every list of that query, its block
 * of out_scores left unwritten, the others served.  Checked before anything is launched, the lambda_q step included: the
 * single-tau forms' checks with their codes and messages, a NaN or infinite tau anywhere in the list and a null taus with ntau > 0
 * -> AS_EINVAL; every finite tau is served.  ntau == 0 and b == 0 launch nothing (ntau == 0: no lambda_q step either); empty lists
 * still run the lambda_q step.  Taus equal by bit pattern are computed once, their rows / lists copied.  The taus per gather
 * (<= 8) and the queries per chunk follow from the "subset_batch_mib" budget (a list too long for it: a chunk of its own, one tau
 * per gather); results never depend on either.  One selection block per (list, tau) pair, one stream wait per (chunk, tau group).
 * The buffers are the single-tau forms' (in the space, grown on demand); calls are serialised with them, as_search runs beside
 * them.  Under "lists_timing" as_lists_kernel_us reports the sweep's score kernel summed over the launches of the call. */
as_status as_score_lists_batch_taus(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d,
                                    const double* taus, int64_t ntau, const int64_t* ids_host, const int64_t* offsets_host,
                                    double* out_scores, double* out_lambda_q, int32_t* out_status);
as_status as_search_lists_batch_taus(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d,
                                     const double* taus, int64_t ntau, const int64_t* ids_host, const int64_t* offsets_host,
                                     int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status);
/* out[0] calls of the two sweeps above that passed their checks, [1] score-kernel launches they made, [2] (query, item) pairs those
 * launches gathered (once per launch, not per tau), [3] (query, item, tau) scores they wrote, [4] lambda_q steps run, [5]
 * (measurement) host nanoseconds spent on id checks, deduplication and work tables.  as_lists_counters counts the single-tau forms
 * only. */
as_status as_lists_sweep_counters(const as_space* sp, int64_t* out, int32_t n);
/* ---- Extension: range search.  EVERY item of a subset (sub == NULL: every item of the space) whose S11 score is >= min_score, by
 * (score descending, index ascending; +0.0 and -0.0 tie), not cut at topk; a NaN score never qualifies; min_score may be -inf
 * (every item whose score is not NaN) or +inf.  The size of the answer is not known before the call, so it comes back as a handle
 * in HOST memory (as_range), independent of the space's lifetime, freed by the caller with as_range_free; count_only != 0: the
 * lists' lengths alone (as_range_offsets; as_range_copy -> AS_EINVAL).  As for the other filtered forms the subset restricts the
 * answer, not the index.  as_search_range: the score of item i has the bits as_score_items returns for it, compared with an IEEE
 * >= in fp64.  as_search_range_batch: b queries, row-major [b][d] in HOST memory, one threshold per query; list i has
 * as_score_items_batch's bits (within 1e-12 relative of the single form's: membership differs from it only for scores that close
 * to the threshold).  Checked before anything is launched: a null argument ("<name>: null argument", *out left NULL), a NaN
 * threshold, a subset of another space, wrong d, a non-finite tau -> AS_EINVAL; a shard of a row-sharded index -> AS_EUNSUPPORTED.
 * Cost: ONE ORDINARY as_search (batched: ONE as_search_batch over all b queries) for lambda_q, hits discarded: the same escalation
 * and the same AS_EZEROLAMBDA whatever the subset and the threshold (batched: in out_status[i], that query gets an empty list, the
 * others are served); then the filtered forms' gather of the subset's rows (batched: once per 64 queries, in chunks of queries
 * under the "subset_batch_mib" budget) and ONE compaction kernel per call (per chunk) that reads the scores once and appends a
 * 16-byte entry per survivor to one buffer: only survivors cross to the host, where each list is sorted (std::sort: the cost
 * grows with the answer -- min_score = -inf over a million items is legal and slow).  If the survivors exceed the buffer (65 536
 * entries at first, grown on demand) the compaction alone is run again, never the gather; count_only never runs it twice.  An
 * empty subset still runs the lambda_q step; b == 0 launches nothing and returns an answer of 0 lists.  sub == NULL: the space
 * makes a subset of all items on first use and keeps it (4 bytes per item, plus the scores).  The buffers live in the subset
 * handle (sub == NULL: in the space) and grow on demand; calls are serialised with as_search_subset on that handle, as_search runs
 * beside them.  out_lambda_q and out_status may be NULL. */
typedef struct as_range as_range;
as_status as_search_range(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, double min_score,
                          const as_subset* sub, int32_t count_only, as_range** out, double* out_lambda_q);
as_status as_search_range_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                const double* min_scores, const as_subset* sub, int32_t count_only, as_range** out,
                                double* out_lambda_q, int32_t* out_status);
int64_t as_range_queries(const as_range* r);                  /* lists: 1, or b; 0 for NULL */
int64_t as_range_total(const as_range* r);                    /* survivors over all lists; 0 for NULL */
as_status as_range_offsets(const as_range* r, int64_t* out);  /* as_range_queries + 1 entries: list i is [out[i], out[i + 1]) */
as_status as_range_copy(const as_range* r, int64_t* out_idx, double* out_score);  /* as_range_total entries; AS_EINVAL after count_only */
void as_range_free(as_range* r);                              /* NULL: no-op */
/* out[0] calls of the two entries above that passed their checks, [1] compaction launches, [2] scores examined, [3] survivors
 * returned (count_only: counted), [4] compaction relaunches after the append buffer overflowed, [5] lambda_q steps run */
as_status as_range_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement: the device microseconds of the compaction kernel, summed over the launches of the last range call on this space
 * that ran under as_set_tuning("range_timing", 1) (HIP events around the kernel; off by default) */
double as_range_kernel_us(const as_space* sp);
/* ---- Extension: diversified search (greedy maximal marginal relevance).  The POOL is the hit list of the ordinary
 * route in its order (score descending, index ascending): as_search's, or as_search_subset's with sub != NULL; batched:
 * as_search_batch's / as_search_subset_batch's lists.  Its size P is at most the index's topk: build with topk = the pool you
 * want, <= 1024.  With g(i, j) the cosine of items i and j (fp64 dot of the rows the filtered forms gather over the square root of
 * the product of the stored squared norms; 0 when that product is 0; not clamped: negative cosines count), r_p the largest g of
 * pool entry p with an entry picked so far (0 while nothing is picked) and s_p its score, step t = 0 .. min(n, P) - 1 picks the
 * unselected p with the largest margin m_p = (1 - diversity) s_p - diversity r_p in fp64; ties go to the smallest p, a NaN margin
 * counts as -inf.  Entry t of the answer: out_idx[t] the item, out_score[t] its S11 score with the route's bits, out_margin[t]
 * (out_margin may be NULL) the margin it was picked with; *out_len = min(n, P).  diversity == 0 returns the first min(n, P) pool
 * entries bit for bit; the first pick is always pool entry 0; n >= P returns the whole pool in MMR order.  The outputs hold
 * min(n, topk') entries (topk' = min(topk, nitems), with a subset min(topk', |S|)); the batched form writes list i at stride
 * nn = min(n, topk') and out_len[i].
 * Checked before anything is launched: a null argument ("<name>: null argument", nothing written), n < 1, a diversity that is NaN
 * or outside [0, 1], a subset of another space, wrong d, a non-finite tau -> AS_EINVAL; a shard of a row-sharded index ->
 * AS_EUNSUPPORTED (codes and messages of as_search_subset).  Cost: ONE ordinary search of the route per call (batched: ONE batched
 * search over all b queries): the pool, lambda_q, the escalations and AS_EZEROLAMBDA are that call's (batched: in out_status[i],
 * that query gets out_len 0, the others are served); then per chunk of queries ("diverse_chunk", default 4096; <= 0: the default;
 * results never depend on it) one upload of the pools, ONE launch in which a block per query runs the whole greedy -- per step
 * the cosines of the unselected rows with the row just picked, (min(n, P) - 1) P row reads at most, no P x P matrix -- one
 * download and one stream wait.  b == 0 launches nothing.  The buffers live in the space and grow on demand; the selection steps
 * of calls on one space are serialised, as_search runs beside them.  out_lambda_q and out_status may be NULL. */
as_status as_search_diverse(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, int64_t n, double diversity,
                            const as_subset* sub, int64_t* out_idx, double* out_score, double* out_margin, int64_t* out_len,
                            double* out_lambda_q);
as_status as_search_diverse_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau, int64_t n,
                                  double diversity, const as_subset* sub, int64_t* out_idx, double* out_score, double* out_margin,
                                  int64_t* out_len, double* out_lambda_q, int32_t* out_status);
/* out[0] calls of the two entries above that passed their checks, [1] select launches, [2] picks made, [3] item-item dots computed,
 * [4] pool steps run (ordinary searches, single or batched) */
as_status as_diverse_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement: the device microseconds of the select kernel, summed over the chunks of the last diversified call on this space
 * that ran under as_set_tuning("diverse_timing", 1) (HIP events around the kernel; off by default) */
double as_diverse_kernel_us(const as_space* sp);
/* ---- Extension: graph-diffusion search.  The hit list of the ordinary route (as_search, or
 * as_search_subset with `sub`; batched: as_search_batch / as_search_subset_batch) seeds y (y[c_p] = s_p, entries with a non-finite
 * score left out), and f <- fl(fl(alpha * S f) + fl((1 - alpha) * y)) runs `steps` times from f = y over the WHOLE item graph,
 * S = -lap over the stored off-diagonal entries, each row summed in CSR order, every product and sum rounded once.  The search
 * forms return the first min(topk, |sub|) items of `sub` (NULL: every item) by (f descending, index ascending) as (index, f),
 * lists at stride min(topk, n, |sub|); the score form writes f at the m listed ids ([b][m], caller's order, duplicates kept; b = 1
 * serves a single query); as_diffuse_seeds takes the seeds themselves -- query i's are the entries offsets_host[i] ..
 * offsets_host[i + 1] - 1 of ids_host / values_host, ids distinct per query and inside [0, n), values finite -- and writes the whole
 * f, [b][n] doubles: the whole block crosses to the host.  Refused before anything is launched, the route's search included:
 * alpha outside [0, 1) or NaN, steps outside [0, 64], bad ids or seeds (AS_EINVAL); a feature-mode graph, a row-sharded graph or
 * space (AS_EUNSUPPORTED).  A zero lambda_q: the single form returns AS_EZEROLAMBDA as as_search does; in the batched forms that
 * query gets out_len 0 / a row of NaN and status AS_EZEROLAMBDA, the others are served.  The buffers (two f blocks of n x C
 * doubles, C = 1, 16 or 64 columns per chunk within the "diffuse_mib" budget, default 1024 MiB for the pair: 64 columns up to 1M items) live in the space and
 * grow on demand; the recurrences of calls on one space are serialised, as_search runs beside them.  out_lambda_q and out_status
 * may be NULL.  Tunings (as_set_tuning; results never depend on them): "diffuse_mib", "diffuse_cols" (columns of a chunk at most),
 * "diffuse_tile_edges" (edges of an LDS tile of the one-column kernel), "diffuse_grid_cap" (clips the step kernels' grids),
 * "diffuse_timing" = 1 / 0. */
as_status as_search_diffuse(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, double alpha, int64_t steps,
                            const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q);
as_status as_search_diffuse_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau, double alpha,
                                  int64_t steps, const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len,
                                  double* out_lambda_q, int32_t* out_status);
as_status as_score_diffuse_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau, double alpha,
                                 int64_t steps, const int64_t* ids_host, int64_t m, double* out_scores, double* out_lambda_q,
                                 int32_t* out_status);
as_status as_diffuse_seeds(const as_space* sp, const as_graph* gr, const int64_t* ids_host, const double* values_host,
                           const int64_t* offsets_host, int64_t b, double alpha, int64_t steps, double* out_f);
/* out[0] calls of the four entries above that passed their checks, [1] route searches run (single or batched), [2] column chunks,
 * [3] step launches, [4] seeds uploaded */
as_status as_diffuse_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement: the device microseconds of the steps (step and seed kernels), summed over the chunks of the last diffusion call on
 * this space that ran under as_set_tuning("diffuse_timing", 1) (HIP events around them; off by default) */
double as_diffuse_kernel_us(const as_space* sp);
/* ---- Extension: fixed-point diffusion search.  The four forms above with the fixed point of the
 * recurrence in place of `steps` steps: f = (1 - alpha) (I - alpha S)^-1 y by conjugate gradients on the device, per query and
 * independent of every other query, started from 0 and stopped when r.r <= fl(fl(tol tol) b.b), after max_iters iterations, or
 * when p.(I - alpha S)p is not > 0 (a breakdown; x is kept).  The seeds, the pool, S, the subset rule, the zero-lambda rule and the
 * answer shapes are those of the forms above; every product, sum, difference and quotient is rounded once and the one reduction
 * (64-row segments in row order, then a halving tree) has a fixed order, so the answer, the iteration count and the residual have
 * the bits of the numpy reference whatever the column chunk, the tile or the grid.  Per query (each pointer may be NULL; [b], or one
 * entry of the single form): out_iters the iterations run, out_residual sqrt(r.r / b.b) at the stop (0 for y = 0; NaN for a query
 * that was not served), out_state 1 converged / 0 stopped at max_iters (or not served) / 2 breakdown.  A query that does not
 * converge is served with the x it has; that is no error.  Refused before anything is launched: alpha outside [0, 1), tol not
 * finite or <= 0, max_iters outside [1, 1024] (AS_EINVAL), and what the forms above refuse.  The four vectors x, r, p, q of n x C
 * doubles stay within "diffuse_solve_mib" (default 2048 MiB: the column widths of "diffuse_mib"); "diffuse_cols",
 * "diffuse_tile_edges", "diffuse_grid_cap" and "diffuse_timing" hold as above. */
as_status as_search_diffuse_solve(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, double alpha, double tol,
                                  int64_t max_iters, const as_subset* sub, int64_t* out_idx, double* out_score, int64_t* out_len,
                                  double* out_lambda_q, int32_t* out_iters, double* out_residual, int32_t* out_state);
as_status as_search_diffuse_solve_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                        double alpha, double tol, int64_t max_iters, const as_subset* sub, int64_t* out_idx,
                                        double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status, int32_t* out_iters,
                                        double* out_residual, int32_t* out_state);
as_status as_score_diffuse_solve_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                       double alpha, double tol, int64_t max_iters, const int64_t* ids_host, int64_t m, double* out_scores,
                                       double* out_lambda_q, int32_t* out_status, int32_t* out_iters, double* out_residual,
                                       int32_t* out_state);
as_status as_diffuse_solve_seeds(const as_space* sp, const as_graph* gr, const int64_t* ids_host, const double* values_host,
                                 const int64_t* offsets_host, int64_t b, double alpha, double tol, int64_t max_iters, double* out_f,
                                 int32_t* out_iters, double* out_residual, int32_t* out_state);
/* out[0] calls of the four entries above that passed their checks, [1] route searches run, [2] column chunks, [3] iterations
 * launched (per chunk: the largest iteration count of its columns), [4] host waits of the iteration loops (one at the start of a
 * chunk, one per iteration), [5] seeds uploaded */
as_status as_diffuse_solve_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement, of the last solve on this space that ran under as_set_tuning("diffuse_timing", 1), summed over its chunks (HIP
 * events): part 0 the device microseconds from the first to the last launch of the iterations (the host's waits between them
 * included); parts 1 .. 5 the five launches of ONE sampled iteration per chunk (its second, or its only one): the apply kernel,
 * the reduce of p.q, the update kernel, the reduce of r.r, the direction kernel (with the copy of the scalars ahead of it) */
double as_diffuse_solve_kernel_us(const as_space* sp, int32_t part);
/* ---- Extension: graph eigenpairs.  The m largest eigenvalues of S (the operator of the diffusion
 * forms above: the stored off-diagonal entries of `lap`, negated) and their eigenvectors, by block Chebyshev-filtered subspace
 * iteration with Rayleigh-Ritz on the device: a block of C = 16 (m <= 12) or 64 columns, all iterated every time, from a start
 * block that `seed` fixes.  out_values [m], descending (for a row with an edge, 1 - value is the normalised Laplacian's
 * eigenvalue); out_vectors [m][n], orthonormal, row j belonging to out_values[j], its entry of largest magnitude (lowest index on
 * ties) positive; out_residuals [m], |S v - theta v|_2 as the device formed it; out_info [4]: outer iterations, state (1: every
 * wanted residual <= tol; 0: stopped at max_iters, the iterate it has is served; 2: the block lost a direction -- a Gram
 * eigenvalue <= 1e-14 of the largest -- and values, vectors and residuals are not written), step launches, C.  An outer iteration:
 * Y = S X, H = X^T Y, the host decomposes H (a cyclic Jacobi, no LAPACK), X <- X Q, Y <- Y Q, the residuals; then a Chebyshev
 * filter of at most `degree` steps over [-1, cut], cut below the smallest Ritz value and at least 1e-3 (theta_1 + 1) below the
 * largest, its growth capped at 2e6, and two orthonormalisations (G = X^T X = U L U^T, X <- X U L^-1/2).  The four device
 * primitives (step, gram, rotate, colnorm2) have fixed orders and round every product and sum once: each has the bits of the numpy
 * reference; the driver's answer depends on the host eigensolver's roundings and is checked by what an eigenpair must satisfy.  The
 * same call returns the same bits, whatever "diffuse_grid_cap".  Refused before anything is launched: m outside [1, 48], tol not in
 * (0, 1), max_iters outside [1, 10000], degree outside [1, 64], seed < 0, n < C, four n x C blocks beyond the "spectral_mib" budget
 * (default 8192 MiB) (AS_EINVAL); a feature-mode or row-sharded graph (AS_EUNSUPPORTED).  The blocks are the diffusion forms' work
 * buffers: calls on one space are serialised with them. */
as_status as_graph_eigs(const as_space* sp, const as_graph* gr, int64_t m, double tol, int64_t max_iters, int64_t degree, int64_t seed,
                        double* out_values, double* out_vectors, double* out_residuals, int64_t* out_info);
/* out[0] calls that passed their checks, [1] outer iterations, [2] step launches, [3] Gram launches, [4] rotate launches, [5] host
 * waits (one per Gram, one per residual, one for the answer) */
as_status as_graph_eigs_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement, of the last as_graph_eigs on this space: part 0 the call's wall microseconds, 5 the host eigensolver's, 6 the
 * host's waits; under as_set_tuning("diffuse_timing", 1) parts 1 .. 4 the device microseconds (HIP events around every launch,
 * which then run one at a time) of the steps, the Grams with their trees, the rotates, and colnorm2 with its tree */
double as_graph_eigs_kernel_us(const as_space* sp, int32_t part);
/* debug: one S21 primitive on host blocks, through exactly the launch as_graph_eigs makes.  Blocks are [n][C] doubles, C = 16 or 64.
 * AS_SPECTRAL_STEP (n the graph's): out = fl(fl(fl(a acc) + fl(b V)) + fl(g W)) with V = a_host, W = b_host (NULL with g == 0),
 * coef = {a, b, g, alias}; alias != 0: the result is written over W's block.  AS_SPECTRAL_GRAM: out [C][C] = A^T B (b_host NULL:
 * B = A).  AS_SPECTRAL_ROTATE: out [n][C] = X T, t_host = T [C][C].  AS_SPECTRAL_COLNORM2: out [C], the squared column norms of
 * Y - X theta with X = a_host, Y = b_host, t_host = theta [C]. */
enum { AS_SPECTRAL_STEP = 0, AS_SPECTRAL_GRAM = 1, AS_SPECTRAL_ROTATE = 2, AS_SPECTRAL_COLNORM2 = 3 };
as_status as_spectral_op(const as_space* sp, const as_graph* gr, int32_t op, int64_t n, int32_t C, const double* a_host, const double* b_host,
                         const double* t_host, const double* coef, double* out_host);
/* the host eigensolver of as_graph_eigs (no GPU): a symmetric n x n matrix, row-major -> w [n] ascending, v [n][n] row-major with
 * eigenvector j in column j.  -> the Jacobi sweeps run, -1 on a bad argument or if 64 sweeps did not end it */
int32_t as_sym_eig_host(const double* a, int32_t n, double* w, double* v);
/* ---- Extension: connected components of the item graph.  The stored CSR of a whole item graph is
 * used (no diagonal; `dist` per entry).  Kept entries: max_dist == NULL: every stored entry; else the entries with dist <= *max_dist
 * (a NaN dist is never kept under a threshold; +inf keeps every entry whose dist is no NaN, -inf none).  Items i and j are joined iff
 * at least one of the stored entries i -> j, j -> i is kept; the components are the classes of the transitive closure; the label
 * of an item is the smallest item id of its component (an item without a kept entry is its own label).  labels_host [n] int32.
 * info (may be NULL): the components, the size of the largest, the smallest label of that size, the components of one item, the
 * stored entries kept (both directions as stored) and the rounds run -- every field but `rounds` is a function of the graph and
 * the threshold alone.  On the device: parent[i] = i, then rounds of two launches -- hook (for a kept entry (i, j) with
 * a = parent[i] != b = parent[j]: atomicMin(&parent[max(a, b)], min(a, b))) and compress (every item stores its root) -- until the
 * host reads that a round's hook met no entry with unequal parents; `rounds` counts the hook launches.  Sizes and the four
 * statistics are formed on the device with integer atomics; six numbers cross per threshold, and as_graph_components alone copies
 * the labels.  The answer does not depend on "diffuse_grid_cap" nor on the order in which the atomics land.
 * as_graph_components_sweep: nt thresholds in [1, 64], any order, duplicates allowed -> info [nt] in the caller's order; the
 * distinct thresholds run ascending, each from the labels of the one before (the kept sets are nested); no labels cross.
 * Refused before anything is launched: a NaN threshold, nt outside [1, 64], a graph whose row count is not the space's (AS_EINVAL);
 * a feature-mode or row-sharded graph (AS_EUNSUPPORTED).  The buffers are the diffusion forms' workspace: calls on one space are
 * serialised with them. */
typedef struct as_components_info {
    int64_t count;          /* components */
    int64_t largest;        /* items of the largest component */
    int64_t largest_label;  /* the smallest label whose component has that size */
    int64_t isolated;       /* components of one item */
    int64_t edges_kept;     /* stored entries kept, both directions as stored */
    int64_t rounds;         /* hook launches */
} as_components_info;
as_status as_graph_components(const as_space* sp, const as_graph* gr, const double* max_dist, int32_t* labels_host, as_components_info* info);
as_status as_graph_components_sweep(const as_space* sp, const as_graph* gr, const double* max_dists, int32_t nt, as_components_info* info);
/* out[0] calls that passed their checks, [1] thresholds served (1 for a call without one), [2] hook launches, [3] compress
 * launches, [4] host waits (one per round, one per stage for the statistics) */
as_status as_components_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement, of the last components call on this space under as_set_tuning("diffuse_timing", 1): part 0 the device microseconds
 * of its hook launches, 1 of its compress launches, 2 of its statistics (sizes and reduction); part 3 its rounds (any timing) */
double as_components_kernel_us(const as_space* sp, int32_t part);
/* ---- Extension: fused multi-query search.  ONE answer to j >= 1 query vectors, row-major [j][d] in HOST memory,
 * with finite weights w (weights == NULL: 1/j each; negative weights are legal).  s_v(i): the S11 score of item i for vector v
 * with the bits as_score_items_batch writes at [v][i] (lambda_q of every vector from ONE as_search_batch over the j vectors, the
 * dot from the batched score kernel).  t_v(i) = fl(w_v * s_v(i)), one rounded multiply.  Over the SERVED vectors, v ascending:
 * mode 0 (sum): F = t of the first served vector, then F = fl(F + t_v), every sum rounded once, no FMA; mode 1 (max): F = t of
 * the first served vector, then F = t_v if (t_v > F or F is NaN), else F -- the first largest term wins, a NaN never displaces a
 * number, F is NaN only if every term is.  A vector whose lambda_q is 0: skip_zero == 0: the whole call returns
 * AS_EZEROLAMBDA and no answer is written; skip_zero != 0: that vector is left out, its weight is dropped and the others are not
 * renormalised; if no vector is served the call returns AS_EZEROLAMBDA in either setting.  out_lambda_q / out_status ([j] each,
 * may be NULL) are written whenever the lambda_q step ran.
 * as_search_fused: the first min(topk', |sub|) items of the subset (sub == NULL: every item; topk' = min(topk, nitems)) by (F
 * descending, index ascending; +0.0 and -0.0 tie) -> out_idx / out_score, *out_len.  as_score_fused: F of every listed id ->
 * out_scores[m], the caller's order, duplicates kept.  With j == 1 and w = {1.0} the search form returns list 0 of
 * as_search_subset_batch bit for bit in both modes.
 * Checked before anything is launched: a null argument ("<name>: null argument", nothing written), j <= 0, a mode other than 0 / 1,
 * a NaN or infinite weight, a subset of another space, wrong d, a non-finite tau, an id outside [0, nitems) -> AS_EINVAL; a shard
 * of a row-sharded index -> AS_EUNSUPPORTED.  Cost: ONE as_search_batch over the j vectors (hits discarded), then per chunk of
 * vectors under the "subset_batch_mib" budget the batched filtered forms' gather and fp64 matrix product, whose [chunk][m] scores
 * stay on the device, and ONE accumulate kernel that reads them once and folds them into an accumulator of m doubles, which
 * carries over the chunks; at the end the filtered forms' exact selection over the accumulator (the search form: topk' entries
 * cross to the host) or one copy of its m doubles (the score form).  An empty subset or m == 0 still runs the lambda_q step and
 * returns an empty answer.  The buffers live in the subset handle (sub == NULL: in the space's subset of all items, made on first
 * use; the score form: in the space's as_score_items buffers) and grow on demand; calls are serialised with the other forms on
 * that handle, as_search runs beside them. */
as_status as_search_fused(const as_space* sp, const as_graph* gr, const double* queries, int64_t j, int64_t d, double tau,
                          const double* weights, int32_t mode, int32_t skip_zero, const as_subset* sub, int64_t* out_idx,
                          double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status);
as_status as_score_fused(const as_space* sp, const as_graph* gr, const double* queries, int64_t j, int64_t d, double tau,
                         const double* weights, int32_t mode, int32_t skip_zero, const int64_t* ids_host, int64_t m, double* out_scores,
                         double* out_lambda_q, int32_t* out_status);
/* out[0] calls of the two entries above that passed their checks, [1] accumulate launches, [2] scores folded (served rows x m),
 * [3] lambda_q steps run */
as_status as_fused_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement: the device microseconds of the accumulate kernel, summed over the chunks of the last fused call on this space that
 * ran under as_set_tuning("fused_timing", 1) (HIP events around the kernel; off by default) */
double as_fused_kernel_us(const as_space* sp);
/* ---- Extension: batched fused search.  b >= 1 NEEDS in one call: need y is the vectors offsets[y] ..
 * offsets[y + 1] - 1 of the nv flattened query vectors ([nv][d], HOST memory), J_y = offsets[y + 1] - offsets[y] >= 1 of them, with
 * the flattened finite weights weights[nv] (NULL: 1/J_y each inside need y).  offsets: int64 [b + 1], starts at 0, increases
 * strictly, ends at nv.  tau, mode, skip_zero and the subset / the ids are common to the call.  The per-vector scores are the
 * bits as_score_items_batch writes for the nv vectors (lambda_q of every vector from ONE as_search_batch over all nv); need y's F
 * is the fold of as_search_fused over ITS rows, ascending, every product and sum rounded once.  b == 1 is as_search_fused /
 * as_score_fused bit for bit.
 * A vector whose lambda_q is 0: skip_zero == 0: the whole call returns AS_EZEROLAMBDA before any gather is launched and no answer
 * is written; skip_zero != 0: it is left out of its need (the other weights are not renormalised); a need with no vector left is
 * not served -- out_len[y] = 0 / a row of NaN -- and the call still returns AS_OK, also when no need at all is served (nothing is
 * launched then).  out_status ([b], may be NULL): 0 or AS_EZEROLAMBDA per NEED (skip_zero == 0: a need that holds such a
 * vector); out_lambda_q ([nv], may be NULL): per flattened vector; both are written whenever the lambda_q step ran.
 * as_search_fused_batch: need y's first min(topk', |sub|) items by (F descending, index ascending) -> out_idx / out_score +
 * y * hits_bound, out_len[y], hits_bound = min(topk, nitems, |sub|) (sub == NULL: every item).  as_score_fused_batch: F of every
 * listed id -> out_scores[y * m + i], the caller's order, duplicates kept.
 * Checked before any handle is touched, with nothing written: a null argument ("<name>: null argument"), b < 1, offsets that do
 * not start at 0, increase strictly and end at nv -> AS_EINVAL.  Then as as_search_fused: mode, weights, the subset's space, d,
 * tau, ids -> AS_EINVAL; a shard of a row-sharded index -> AS_EUNSUPPORTED.
 * Cost: ONE as_search_batch over the nv vectors; then the needs are taken G at a time, G = the accumulator rows of m doubles that
 * fit the "fused_batch_mib" budget (1 <= G <= 4096): the group's vectors go through the batched filtered forms' gather and fp64
 * matrix product as ONE list of rows in chunks under "subset_batch_mib", ONE segmented accumulate kernel per chunk folds every
 * need's rows of the chunk into that need's accumulator row, and after the group's last chunk one batched exact selection (the
 * search form) or one copy of the rows (the score form) follows.  Answers never depend on G, the chunks or the grid.  The
 * buffers are those of the single forms. */
as_status as_search_fused_batch(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                                int64_t d, double tau, const double* weights, int32_t mode, int32_t skip_zero, const as_subset* sub,
                                int64_t* out_idx, double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status);
as_status as_score_fused_batch(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                               int64_t d, double tau, const double* weights, int32_t mode, int32_t skip_zero, const int64_t* ids_host,
                               int64_t m, double* out_scores, double* out_lambda_q, int32_t* out_status);
/* out[0] calls of the two entries above that passed their checks, [1] needs of those calls, [2] accumulate launches, [3] scores
 * folded (served rows x m), [4] lambda_q steps run (one per call), [5] need groups run */
as_status as_fused_batch_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement: the device microseconds of the segmented accumulate kernel, summed over the chunks of the last batched fused call
 * on this space that ran under as_set_tuning("fused_batch_timing", 1) (HIP events around the kernel; off by default) */
double as_fused_batch_kernel_us(const as_space* sp);
/* ---- Extension: grouped search.  The best items of the best groups.  as_groups_create: one int64 label per item
 * of the space (labels[n], n == nitems, HOST memory, any values; equal labels = one group) -> a handle; the labels are turned into
 * dense group numbers (ascending label) on the host and uploaded once.  as_groups_count: distinct labels.
 * s(i): the S11 score of item i with the bits as_score_items (single form) / as_score_items_batch (batched form) writes.  Items
 * are ordered by (score descending, index ascending; +0.0 and -0.0 tie); an item whose score is NaN belongs to no answer.  A
 * group's MEMBERS are its items inside the subset (sub == NULL: every item) with a non-NaN score, in that order; its HEAD is the
 * first; a group without a member does not exist for the call.  Groups are ordered by their heads in the item order (two groups
 * never tie).  The answer: the first min(n_groups, groups with a member) groups -> *out_ngroups; for group s its label ->
 * out_label[s], its first min(per_group, members) members -> out_count[s] and out_idx / out_score[s * per_group + t].  The
 * subset restricts the answer, not the index: lambda_q and the items' lambdas are the ones as_search uses.
 * as_search_grouped: lambda_q == 0 -> AS_EZEROLAMBDA, whatever the labels and the subset.  as_search_grouped_batch: b queries
 * [b][d]; query i's outputs at out_label / out_count + i * n_groups, out_idx / out_score + i * n_groups * per_group,
 * out_ngroups[i]; a query whose lambda_q is 0 gets out_status[i] == AS_EZEROLAMBDA and 0 groups, the others are served.
 * out_lambda_q / out_status (may be NULL) are written whenever the lambda_q step ran.
 * Checked before anything is launched: a null argument ("<name>: null argument", nothing written), n_groups outside [1, 1024],
 * per_group outside [1, 16], a groups handle or a subset of another space, wrong d, a non-finite tau -> AS_EINVAL; a shard of a
 * row-sharded index -> AS_EUNSUPPORTED.
 * Cost: one as_search (batched: ONE as_search_batch over the b queries), hits discarded; the filtered forms' gather and score
 * kernel, whose scores stay on the device; per round two pick launches that each read the scores (8 bytes) and the subset's
 * ids and group numbers (4 to 8 bytes) of every position and issue one vector atomic per run of neighbouring positions of one
 * group inside a wave; one collapse launch and the filtered forms' exact selection over the heads; per_group - 1 further rounds
 * over the selected groups (fewer when no selected group is that large); one gather launch, one copy.  Two waits (one when
 * per_group == 1).  The batched form works in chunks of queries under the "subset_batch_mib" budget, which counts the scores, the
 * collapsed scores and the per-group cells of a query.  The buffers live in the subset handle (sub == NULL: in the space's
 * subset of all items, made on first use) and grow on demand; calls are serialised with the other forms on that handle,
 * as_search runs beside them. */
typedef struct as_groups as_groups;
as_status as_groups_create(const as_space* sp, const int64_t* labels, int64_t n, as_groups** out);
int64_t as_groups_count(const as_groups* g);                  /* NULL: 0 */
void as_groups_free(as_groups* g);                            /* NULL: no-op */
as_status as_search_grouped(const as_space* sp, const as_graph* gr, const double* query, int64_t d, double tau, const as_groups* groups,
                            int64_t n_groups, int64_t per_group, const as_subset* sub, int64_t* out_label, int64_t* out_count,
                            int64_t* out_idx, double* out_score, int64_t* out_ngroups, double* out_lambda_q);
as_status as_search_grouped_batch(const as_space* sp, const as_graph* gr, const double* queries, int64_t b, int64_t d, double tau,
                                  const as_groups* groups, int64_t n_groups, int64_t per_group, const as_subset* sub,
                                  int64_t* out_label, int64_t* out_count, int64_t* out_idx, double* out_score, int64_t* out_ngroups,
                                  double* out_lambda_q, int32_t* out_status);
/* out[0] calls of the two entries above that passed their checks, [1] pick-kernel launches, [2] scores examined (queries x m per
 * pick launch), [3] 64-bit max-atomics the pick kernels issued, [4] groups returned, [5] members returned, [6] lambda_q steps run */
as_status as_grouped_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement: the device microseconds of the pick kernels, summed over the rounds and chunks of the last grouped call on this
 * space that ran under as_set_tuning("grouped_timing", 1) (HIP events around the kernels; off by default) */
double as_grouped_kernel_us(const as_space* sp);
/* ---- Extension: late-interaction search (MaxSim).  ONE answer to j query vectors [j][d] (HOST memory) over the
 * GROUPS of an as_groups handle: with s_j(i) the bits as_score_items_batch writes at [j][i], m_j(g) = the largest s_j over the
 * members of g -- its items inside the subset (sub == NULL: every item) whose s_j is not NaN; +0.0 where the largest is a zero;
 * NaN where g has no member under vector j -- and F(g) = the S13 "sum" fold of t_j(g) = fl(weights[j] * m_j(g)), j ascending over
 * the served vectors, every product and sum rounded once (weights NULL: 1/j each; finite, negative values are legal).  The
 * zero-lambda rule is as_search_fused's: skip_zero == 0: a vector whose lambda_q is 0 makes the call return AS_EZEROLAMBDA before
 * anything else is launched; skip_zero != 0: it is left out, the other weights are not renormalised; no vector served ->
 * AS_EZEROLAMBDA in either setting.  out_lambda_q / out_status ([j], may be NULL) are written whenever the lambda_q step ran.
 * as_search_maxsim: the groups whose F is not NaN by (F descending, label ascending; +0.0 and -0.0 tie), the first
 * min(n_groups, such groups) of them -> out_label / out_score [n_groups], *out_len.  as_score_maxsim: F of every listed label ->
 * out_scores [nl], the caller's order, duplicates kept, NaN for a group without a member.
 * Checked before anything is launched: a null argument ("<name>: null argument", nothing written), n_groups outside [1, 1024], a
 * groups handle or a subset of another space, a label the handle does not hold, j < 1, a NaN or infinite weight, wrong d, a
 * non-finite tau -> AS_EINVAL; a shard of a row-sharded index -> AS_EUNSUPPORTED.
 * Cost: ONE as_search_batch over the j vectors (hits discarded); per chunk of vectors under the "subset_batch_mib" budget (which
 * counts the 8 G bytes of a vector's cells beside its m scores, G = as_groups_count) the batched filtered forms' gather and fp64
 * matrix product, one memset of the chunk's cells, the first pass of grouped search's pick kernel (one vector atomic per run of
 * neighbouring positions of one group inside a wave) and ONE fold kernel that reads the [chunk][G] cells once and folds them
 * into an accumulator of G doubles, which carries over the chunks; at the end the filtered forms' exact selection over the
 * accumulator (n_groups entries cross to the host) or one copy of its G doubles.  One wait per chunk plus the last.  The buffers
 * live in the subset handle (sub == NULL: in the space's subset of all items, made on first use) and grow on demand; calls are
 * serialised with the other forms on that handle, as_search runs beside them. */
as_status as_search_maxsim(const as_space* sp, const as_graph* gr, const double* queries, int64_t j, int64_t d, double tau,
                           const double* weights, int32_t skip_zero, const as_groups* groups, int64_t n_groups, const as_subset* sub,
                           int64_t* out_label, double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status);
as_status as_score_maxsim(const as_space* sp, const as_graph* gr, const double* queries, int64_t j, int64_t d, double tau,
                          const double* weights, int32_t skip_zero, const as_groups* groups, const as_subset* sub, const int64_t* labels,
                          int64_t nl, double* out_scores, double* out_lambda_q, int32_t* out_status);
/* out[0] calls of the two entries above that passed their checks, [1] vectors served, [2] pass-A launches, [3] 64-bit max-atomics
 * pass A issued, [4] fold launches */
as_status as_maxsim_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement: device microseconds of the last late-interaction call on this space that ran under as_set_tuning("maxsim_timing",
 * 1) (HIP events; off by default), summed over its chunks: part 1: the memsets of the cells and pass A; part 2: the fold kernel;
 * part 0: both.  NULL or another part: 0 */
double as_maxsim_kernel_us(const as_space* sp, int32_t part);
/* ---- Extension: batched late-interaction search.  b >= 1 NEEDS in one call: need y is the vectors offsets[y] ..
 * offsets[y + 1] - 1 of the nv flattened query vectors ([nv][d], HOST memory), J_y = offsets[y + 1] - offsets[y] >= 1 of them, with
 * the flattened finite weights weights[nv] (NULL: 1/J_y each inside need y).  offsets: int64 [b + 1], starts at 0, increases
 * strictly, ends at nv.  tau, skip_zero, the groups, n_groups and the subset are common to the call.  The per-vector scores are
 * the bits as_score_items_batch writes for the nv vectors (lambda_q of every vector from ONE as_search_batch over all nv); m_v(g)
 * is as_search_maxsim's group maximum per flattened vector, and need y's F is the fold of as_search_maxsim over ITS served rows,
 * ascending, every product and sum rounded once.  b == 1 is as_search_maxsim / as_score_maxsim bit for bit.
 * A vector whose lambda_q is 0: skip_zero == 0: the whole call returns AS_EZEROLAMBDA before any gather is launched and no answer
 * is written; skip_zero != 0: it is left out of its need (the other weights are not renormalised); a need with no vector left is
 * not served -- out_len[y] = 0 / a row of NaN -- and the call still returns AS_OK, also when no need at all is served (nothing is
 * launched then).  out_status ([b], may be NULL): 0 or AS_EZEROLAMBDA per NEED (skip_zero == 0: a need that holds such a
 * vector); out_lambda_q ([nv], may be NULL): per flattened vector; both are written whenever the lambda_q step ran.
 * as_search_maxsim_batch: need y's groups whose F is not NaN by (F descending, label ascending; +0.0 and -0.0 tie), the first
 * min(n_groups, such groups) of them -> out_label / out_score + y * n_groups, out_len[y].  as_score_maxsim_batch: F of every
 * listed label -> out_scores[y * nl + l], the caller's order, duplicates kept, NaN for a group without a member.
 * Checked before any handle is touched, with nothing written: a null argument ("<name>: null argument"), b < 1, offsets that do
 * not start at 0, increase strictly and end at nv -> AS_EINVAL.  (From there on a refusal of the search form leaves every
 * out_len[y] == 0 and nothing else written.)  Then as as_search_maxsim: n_groups outside [1, 1024], a groups
 * handle or a subset of another space, a label the handle does not hold, a NaN or infinite weight, wrong d, a non-finite tau ->
 * AS_EINVAL; a shard of a row-sharded index -> AS_EUNSUPPORTED.
 * Cost: ONE as_search_batch over the nv vectors; then the needs are taken Gn at a time, Gn = the accumulator rows of G doubles
 * (G = as_groups_count) that fit the "maxsim_batch_mib" budget (1 <= Gn <= 4096): the group's vectors go through the batched
 * filtered forms' gather and fp64 matrix product as ONE list of rows in chunks under "subset_batch_mib" (which counts the 8 G
 * bytes of a vector's cells beside its m scores); per chunk one memset of the cells, the first pass of grouped search's pick
 * kernel per run of served rows and ONE segmented fold kernel that folds every need's rows of the chunk into that need's
 * accumulator row; after the group's last chunk one batched exact selection over the accumulator rows (the search form: b x
 * n_groups entries cross to the host) or one pick kernel and one copy of the listed F (the score form: b x nl doubles cross).
 * Answers never depend on Gn, the chunks or the grid.  The buffers are those of the single forms. */
as_status as_search_maxsim_batch(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                                 int64_t d, double tau, const double* weights, int32_t skip_zero, const as_groups* groups, int64_t n_groups,
                                 const as_subset* sub, int64_t* out_label, double* out_score, int64_t* out_len, double* out_lambda_q,
                                 int32_t* out_status);
as_status as_score_maxsim_batch(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                                int64_t d, double tau, const double* weights, int32_t skip_zero, const as_groups* groups, const as_subset* sub,
                                const int64_t* labels, int64_t nl, double* out_scores, double* out_lambda_q, int32_t* out_status);
/* out[0] calls of the two entries above that passed their checks, [1] needs of those calls, [2] vectors served, [3] pass-A
 * launches, [4] 64-bit max-atomics pass A issued, [5] fold launches, [6] lambda_q steps run (one per call), [7] need groups run */
as_status as_maxsim_batch_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement: device microseconds of the last batched late-interaction call on this space that ran under
 * as_set_tuning("maxsim_batch_timing", 1) (HIP events; off by default), summed over its chunks: part 1: the memsets of the cells
 * and pass A; part 2: the segmented fold kernel; part 0: both.  NULL or another part: 0 */
double as_maxsim_batch_kernel_us(const as_space* sp, int32_t part);
/* ---- Extension: late-interaction re-ranking of per-need candidate documents.  The needs, weights, tau, skip_zero
 * and groups of as_search_maxsim_batch, but EVERY NEED HAS ITS OWN CANDIDATE GROUPS ("documents") and there is no subset: need y's
 * documents are need_docs[y] .. need_docs[y + 1] - 1 (need_docs: int64 [b + 1], starts at 0, does not decrease; a need may have
 * none), document dd is the group with label doc_label[dd] (strictly ascending inside a need; needs may share labels) and its
 * entries ids[doc_first[dd] .. doc_first[dd + 1]) are ALL the members of that group in ascending item order (doc_first: int64
 * [nd + 1] from 0, nd = need_docs[b]).  All arrays are HOST memory.  The score of vector v of need y and an entry i is the bits
 * as_score_lists_batch writes for the nv flattened vectors, each with its need's entries as its list (the single forms'
 * summation order; lambda_q of every vector from ONE as_search_batch over all nv); m_v(g), F_y(g) and the zero-lambda rule are
 * as_search_maxsim_batch's, the fold over need y's own served vectors.
 * as_search_maxsim_lists: need y's documents whose F is not NaN by (F descending, label ascending), the first min(n_groups, such
 * documents) -> out_label / out_score + y * n_groups, out_len[y].  as_score_maxsim_lists: F of every document -> out_scores[dd]
 * (NaN: every entry scored NaN, or the need is not served).
 * Checked before the lambda_q step: null arguments, the offsets (as_search_maxsim_batch), n_groups outside [1, 1024], groups of
 * another space, need_docs / doc_first that do not start at 0 or decrease, a label that is not one of the groups or out of order,
 * a document that is not exactly its group's members in ascending order -> AS_EINVAL; 2^31 entries or more, a shard of a
 * row-sharded index -> AS_EUNSUPPORTED.
 * Cost: ONE as_search_batch over the nv vectors; then per chunk of needs whose scores (served vectors x entries) fit the
 * "subset_batch_mib" budget one upload, ONE ragged score launch (a block per segment of <= 64 entries and tile of <= T of the need's
 * vectors staged in LDS: every row is gathered once per TILE, not once per vector), one fold launch (a wave per (need, document):
 * maxima and the weighted sum) and the per-query list forms' selection, a block per need; b x n_groups entries (the score form: nd
 * doubles) cross to the host, the scores never do.  Answers never depend on the chunks, the grid, the order of the needs or the
 * other needs' documents (for the same lambda_q).  Calls on one space are serialised with the per-query list forms. */
as_status as_search_maxsim_lists(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                                 int64_t d, double tau, const double* weights, int32_t skip_zero, const as_groups* groups, int64_t n_groups,
                                 const int64_t* need_docs, const int64_t* doc_label, const int64_t* doc_first, const int64_t* ids,
                                 int64_t* out_label, double* out_score, int64_t* out_len, double* out_lambda_q, int32_t* out_status);
as_status as_score_maxsim_lists(const as_space* sp, const as_graph* gr, const double* queries, const int64_t* offsets, int64_t b, int64_t nv,
                                int64_t d, double tau, const double* weights, int32_t skip_zero, const as_groups* groups,
                                const int64_t* need_docs, const int64_t* doc_label, const int64_t* doc_first, const int64_t* ids,
                                double* out_scores, double* out_lambda_q, int32_t* out_status);
/* out[0] calls of the two entries above that passed their checks, [1] needs of those calls, [2] vectors served, [3] score-kernel
 * launches, [4] rows the score kernel was asked to gather (per need: entries x vector tiles), [5] (vector, row) dots, [6] fold
 * launches, [7] lambda_q steps run (one per call), [8] host nanoseconds spent on the document checks and the work tables */
as_status as_maxsim_lists_counters(const as_space* sp, int64_t* out, int32_t n);
/* measurement: device microseconds of the last call of the two entries on this space that ran under
 * as_set_tuning("maxsim_lists_timing", 1) (HIP events; off by default), summed over its chunks: part 1: the score kernel; part 2:
 * the fold kernel; part 3: the selection (the score form: the copy out); part 0: all.  NULL or another part: 0 */
double as_maxsim_lists_kernel_us(const as_space* sp, int32_t part);
/* the score kernel's geometry on this space: *out_tile = T, the vectors of a need one tile stages (from the padded row length: as
 * many as fit 32 KiB of LDS, 32 at most, 1 where one vector does not fit); *out_segment = entries of a segment at most (64) */
as_status as_maxsim_lists_geometry(const as_space* sp, int64_t* out_tile, int64_t* out_segment);

/* ---- index persistence (extension; the reference exposes none): one flat file
 * holding the items, lambdas and graph arrays.  Loading re-ingests the items and uploads the
 * rest; no k-NN work is redone.  opts->device selects the GPU, metric/kernel come from the file. */
as_status as_index_save(const as_space* sp, const as_graph* gr, const char* path);
as_status as_index_load(const char* path, const as_opts* opts, as_space** out_space, as_graph** out_graph);

void as_free_space(as_space* sp);
void as_free_graph(as_graph* gr);

/* ---- misc ---- */
void as_set_debug(int32_t enabled); /* src/helpers.rs:12-14; messages "[pyarrowspace] ..." on stderr */
const char* as_last_error(void);
int32_t as_device_count(void);
const char* as_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ARROWSPACE_HIP_H */
