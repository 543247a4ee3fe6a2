// Graph eigenpairs (section 5.24): the m largest eigenvalues of S = -lap (S19's operator) and their
// eigenvectors by block Chebyshev-filtered subspace iteration with Rayleigh-Ritz.  A block is [N][C] doubles, item-major, C = 16 or
// 64 columns, all iterated every time; the four blocks are the diffusion forms' work buffers (f[0..1], sv[0..1]).  Four device
// primitives, each fixed in bits (tests/spectral_ref.py reproduces them): step (an SpMV over all columns with two scaled block
// terms), gram (C x C sums over the rows: 1 024-row segments in row order, then S20's halving tree), rotate (a block times a C x C
// matrix held in LDS) and colnorm2 (the column norms of Y - X theta by S20's dot, the residual formed on the fly).  The host steers:
// it decomposes the C x C matrices (a cyclic Jacobi below, no LAPACK) and picks the filter's interval from the Ritz values, waiting
// once per Gram and once per residual.  Every product and sum is rounded once.
// Entry points: as_api.hip (as_graph_eigs, as_graph_eigs_counters, as_graph_eigs_kernel_us, as_spectral_op, as_sym_eig_host).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "as_diffuse.hpp"

// S21 rounds every product and every sum once: no multiply of this file may be fused with the add behind it
#pragma clang fp contract(off)

namespace as {

constexpr int SPC_GRAM_SEG = 1024;       // rows of a segment of S21's Gram
constexpr int SPC_DOT_SEG = 64;          // rows of a segment of S20's dot (colnorm2)
constexpr int SPC_GRAM_ROWS = 16;        // rows of an LDS stage of the Gram kernel
constexpr int SPC_ROT_RPT = 4;           // rows a thread of the rotate kernel owns
constexpr int SPC_TREE_THREADS = 1024;
constexpr double SPC_LO = -1.0;          // the lower end of S's spectrum
constexpr double SPC_GAP_FLOOR = 1e-3;
constexpr double SPC_GROWTH = 2.0e6;
constexpr double SPC_BREAKDOWN = 1e-14;

struct SpectralStepArgs {
    const int64_t* indptr;    // [n + 1]
    const int32_t* indices;   // [nnz]
    const double* lap;        // [nnz]: S_e = -lap[e]
    const double* v;          // [n][C]
    const double* w;          // [n][C]; not read with g == 0; may be `out`
    double* out;              // [n][C]; never v
    int64_t n;
    double a, b, g;
};

// step: out = fl(fl(fl(a acc) + fl(b V)) + fl(g W)), acc the S19 row sum.  The shape of diffuse_step_cols_kernel (as_diffuse.hip),
// whose row sum is copied here so that kernel and its launches stay as they are: lanes own columns, the CT lanes of a row read S_e
// and col_e once (a broadcast) and V[col_e][0 .. CT) as one segment; four edges are loaded ahead of the chain.  A lane reads W at
// the cell it writes and nowhere else, so W may be `out`.
template <int CT>
__global__ __launch_bounds__(DIF_THREADS) void spectral_step_kernel(SpectralStepArgs a) {
    constexpr int RPW = 64 / CT;
    const int lane = threadIdx.x & 63, c = lane % CT, sub = lane / CT;
    const int64_t waves = (int64_t)gridDim.x * (DIF_THREADS / 64);
    for (int64_t r0 = ((int64_t)blockIdx.x * (DIF_THREADS / 64) + (threadIdx.x >> 6)) * RPW; r0 < a.n; r0 += waves * RPW) {
        const int64_t row = r0 + sub;
        if (row >= a.n) continue;
        const int64_t rs = a.indptr[row], re = a.indptr[row + 1];
        const double* __restrict__ f = a.v + c;
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
        double o = a.a * acc + a.b * f[row * CT];
        if (a.g != 0.0) o = o + a.g * a.w[row * CT + c];
        a.out[row * CT + c] = o;
    }
}

// gram, first launch: part[s][i][j] = sum over the rows r of segment s, ascending from +0.0, of fl(A[r][i] B[r][j]).  A block takes
// segments (grid-stride); its 256 threads each own a TI x TI tile of (i, j) chains (4 x 4 at C = 64, one chain at C = 16) in
// registers, and the rows come through LDS, SPC_GRAM_ROWS at a time, read from HBM once per block and coalesced.
template <int CT>
__global__ __launch_bounds__(DIF_THREADS) void spectral_gram_kernel(const double* __restrict__ A, const double* __restrict__ B, int64_t n,
                                                                    double* __restrict__ part) {
    constexpr int TI = CT == 64 ? 4 : 1;
    constexpr int PER = CT / TI;             // tiles along j
    static_assert(PER * PER == DIF_THREADS, "one tile per thread");
    __shared__ double sa[SPC_GRAM_ROWS * CT];
    __shared__ double sb[SPC_GRAM_ROWS * CT];
    const int tid = threadIdx.x;
    const int i0 = (tid / PER) * TI, j0 = (tid % PER) * TI;
    const int64_t nseg = (n + SPC_GRAM_SEG - 1) / SPC_GRAM_SEG;
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t first = s * SPC_GRAM_SEG, last = first + SPC_GRAM_SEG < n ? first + SPC_GRAM_SEG : n;
        double acc[TI][TI];
#pragma unroll
        for (int p = 0; p < TI; ++p)
#pragma unroll
            for (int q = 0; q < TI; ++q) acc[p][q] = 0.0;
        for (int64_t r0 = first; r0 < last; r0 += SPC_GRAM_ROWS) {
            const int rows = last - r0 < SPC_GRAM_ROWS ? (int)(last - r0) : SPC_GRAM_ROWS;
            for (int t = tid; t < rows * CT; t += DIF_THREADS) {
                sa[t] = A[r0 * CT + t];
                sb[t] = B[r0 * CT + t];
            }
            __syncthreads();
            for (int r = 0; r < rows; ++r) {
                double av[TI], bv[TI];
#pragma unroll
                for (int p = 0; p < TI; ++p) av[p] = sa[r * CT + i0 + p];
#pragma unroll
                for (int q = 0; q < TI; ++q) bv[q] = sb[r * CT + j0 + q];
#pragma unroll
                for (int p = 0; p < TI; ++p)
#pragma unroll
                    for (int q = 0; q < TI; ++q) acc[p][q] = acc[p][q] + av[p] * bv[q];
            }
            __syncthreads();   // the stage is read before the next one is written
        }
#pragma unroll
        for (int p = 0; p < TI; ++p)
#pragma unroll
            for (int q = 0; q < TI; ++q) part[(s * CT + i0 + p) * CT + j0 + q] = acc[p][q];
    }
}

// S20's halving tree over the nseg partials of `width` independent entries, in place ([nseg][width]; an entry past nseg counts as
// +0.0): the result is row 0.  A block owns `epb` consecutive entries (width is a multiple of epb), its threads split into
// SPC_TREE_THREADS / epb strands over the segments; a level's writes (j < h) never touch its reads of the upper half (j + h >= h).
__global__ __launch_bounds__(SPC_TREE_THREADS) void spectral_tree_kernel(double* part, int64_t nseg, int width, int epb) {
    const int el = threadIdx.x % epb, strand = threadIdx.x / epb, strands = SPC_TREE_THREADS / epb;
    const int64_t e = (int64_t)blockIdx.x * epb + el;
    int64_t P = 1;
    while (P < nseg) P <<= 1;
    for (int64_t h = P >> 1; h >= 1; h >>= 1) {
        const int64_t top = h < nseg ? h : nseg;
        for (int64_t j = strand; j < top; j += strands) {
            const double hi = j + h < nseg ? part[(j + h) * width + e] : 0.0;
            part[j * width + e] = part[j * width + e] + hi;
        }
        __syncthreads();
    }
}

// rotate: out[r][j] = sum_k X[r][k] T[k][j], k ascending from +0.0.  T sits in LDS for the life of the block; a block takes tiles of
// (256 / CT) * 4 rows (grid-stride), staged through LDS; a thread owns column j of four rows: one read of T[k][j] serves four chains.
template <int CT>
__global__ __launch_bounds__(DIF_THREADS) void spectral_rotate_kernel(const double* __restrict__ X, const double* __restrict__ T, int64_t n,
                                                                      double* __restrict__ out) {
    constexpr int SLOTS = DIF_THREADS / CT, TILE = SLOTS * SPC_ROT_RPT;
    extern __shared__ double spc_lds[];
    double* st = spc_lds;              // [CT][CT]
    double* sx = spc_lds + CT * CT;    // [TILE][CT]
    const int tid = threadIdx.x, j = tid % CT, slot = tid / CT;
    for (int t = tid; t < CT * CT; t += DIF_THREADS) st[t] = T[t];
    const int64_t tiles = (n + TILE - 1) / TILE;
    for (int64_t g = blockIdx.x; g < tiles; g += gridDim.x) {
        const int64_t first = g * TILE;
        const int rows = n - first < TILE ? (int)(n - first) : TILE;
        __syncthreads();   // T is loaded; the last tile is read
        for (int t = tid; t < rows * CT; t += DIF_THREADS) sx[t] = X[first * CT + t];
        __syncthreads();
        double acc[SPC_ROT_RPT];
#pragma unroll
        for (int p = 0; p < SPC_ROT_RPT; ++p) acc[p] = 0.0;
        // (a row of the stage past `rows` holds an older tile's values: finite or not, its chain is never stored)
#pragma unroll 8
        for (int k = 0; k < CT; ++k) {
            const double tv = st[k * CT + j];
#pragma unroll
            for (int p = 0; p < SPC_ROT_RPT; ++p) acc[p] = acc[p] + sx[(slot * SPC_ROT_RPT + p) * CT + k] * tv;
        }
#pragma unroll
        for (int p = 0; p < SPC_ROT_RPT; ++p) {
            const int r = slot * SPC_ROT_RPT + p;
            if (r < rows) out[(first + r) * CT + j] = acc[p];
        }
    }
}

// colnorm2, first launch: the segment partials of S20's dot of R = fl(Y - fl(X theta_c)) with itself; the mapping of the solve's
// update kernel: lanes own columns, a group of CT lanes walks a 64-row segment in ascending order.  Nothing but the partials is written.
template <int CT>
__global__ __launch_bounds__(DIF_THREADS) void spectral_colnorm_kernel(const double* __restrict__ X, const double* __restrict__ Y,
                                                                       const double* __restrict__ theta, int64_t n, double* __restrict__ part) {
    constexpr int SPW = 64 / CT;
    const int lane = threadIdx.x & 63, c = lane % CT, sub = lane / CT;
    const double th = theta[c];
    const int64_t nseg = (n + SPC_DOT_SEG - 1) / SPC_DOT_SEG;
    const int64_t waves = (int64_t)gridDim.x * (DIF_THREADS / 64);
    for (int64_t s0 = ((int64_t)blockIdx.x * (DIF_THREADS / 64) + (threadIdx.x >> 6)) * SPW; s0 < nseg; s0 += waves * SPW) {
        const int64_t s = s0 + sub;
        if (s >= nseg) continue;
        const int64_t first = s * SPC_DOT_SEG, last = first + SPC_DOT_SEG < n ? first + SPC_DOT_SEG : n;
        double sigma = 0.0;
#pragma unroll 4
        for (int64_t row = first; row < last; ++row) {
            const int64_t i = row * CT + c;
            const double rv = Y[i] - X[i] * th;
            sigma = sigma + rv * rv;
        }
        part[s * CT + c] = sigma;
    }
}

// the start block: splitmix64's finaliser over the cell's index and the seed, the top 53 bits as a number of [-0.5, 0.5) (exact)
__global__ __launch_bounds__(DIF_THREADS) void spectral_start_kernel(double* __restrict__ x, int64_t cells, uint64_t seed_term) {
    for (int64_t i = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; i < cells; i += (int64_t)gridDim.x * DIF_THREADS) {
        uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull + seed_term;
        z ^= z >> 30;
        z *= 0xBF58476D1CE4E5B9ull;
        z ^= z >> 27;
        z *= 0x94D049BB133111EBull;
        z ^= z >> 31;
        x[i] = (double)(z >> 11) * 0x1.0p-53 - 0.5;
    }
}

// out[c][i] = x[i][c], c < m: the [m][N] layout of the answer
__global__ __launch_bounds__(DIF_THREADS) void spectral_rows_kernel(const double* __restrict__ x, int C, int m, int64_t n, double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * DIF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DIF_THREADS)
        for (int c = 0; c < m; ++c) out[(int64_t)c * n + i] = x[i * C + c];
}

// ------------------------------------------------------------------ host side
static std::atomic<int> g_spectral_mib{SPC_MIB_DEFAULT};
void set_spectral_mib(int v) { g_spectral_mib.store(v > 0 ? v : SPC_MIB_DEFAULT, std::memory_order_relaxed); }
int64_t spectral_budget() { return (int64_t)g_spectral_mib.load(std::memory_order_relaxed) << 20; }
double spectral_kernel_us(const DiffuseWork* w, int part) { return !w || part < 0 || part > 6 ? 0.0 : w->spectral_us[part]; }

// Cyclic Jacobi for a symmetric n x n matrix (row-major `a`, read only): w the eigenvalues ascending, v row-major with eigenvector
// j in column j.  A rotation is skipped once |a_pq| <= eps sqrt(|a_pp a_qq|) (the test that keeps the small eigenvalues of a
// positive definite matrix to relative accuracy) or |a_pq| is below 1e-290 of the matrix's norm (a zero diagonal).  -> the sweeps
// run, -1 if 64 sweeps did not end it (w and v then hold the last iterate) or on a bad argument.
int sym_eig_host(const double* a, int n, double* w, double* v) {
    if (!a || !w || !v || n < 1) return -1;
    std::vector<double> m((size_t)n * n), u((size_t)n * n, 0.0);
    double norm2 = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            m[(size_t)i * n + j] = 0.5 * (a[(size_t)i * n + j] + a[(size_t)j * n + i]);
            norm2 += m[(size_t)i * n + j] * m[(size_t)i * n + j];
        }
    for (int i = 0; i < n; ++i) u[(size_t)i * n + i] = 1.0;
    const double eps = 0x1.0p-53, floor_abs = 1e-290 * std::sqrt(norm2);
    int sweeps = 0;
    bool done = n == 1 || norm2 == 0.0;
    while (!done && sweeps < 64) {
        ++sweeps;
        done = true;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = m[(size_t)p * n + q], app = m[(size_t)p * n + p], aqq = m[(size_t)q * n + q];
                if (std::fabs(apq) <= eps * std::sqrt(std::fabs(app) * std::fabs(aqq)) || std::fabs(apq) <= floor_abs) continue;
                done = false;
                // the rotation that zeroes a_pq: t the smaller root of t^2 + 2 zeta t - 1 = 0
                const double zeta = (aqq - app) / (2.0 * apq);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < n; ++k) {   // columns p and q
                    const double kp = m[(size_t)k * n + p], kq = m[(size_t)k * n + q];
                    m[(size_t)k * n + p] = c * kp - s * kq;
                    m[(size_t)k * n + q] = s * kp + c * kq;
                }
                for (int k = 0; k < n; ++k) {   // rows p and q
                    const double pk = m[(size_t)p * n + k], qk = m[(size_t)q * n + k];
                    m[(size_t)p * n + k] = c * pk - s * qk;
                    m[(size_t)q * n + k] = s * pk + c * qk;
                }
                m[(size_t)p * n + q] = 0.0;
                m[(size_t)q * n + p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double kp = u[(size_t)k * n + p], kq = u[(size_t)k * n + q];
                    u[(size_t)k * n + p] = c * kp - s * kq;
                    u[(size_t)k * n + q] = s * kp + c * kq;
                }
            }
    }
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return m[(size_t)x * n + x] < m[(size_t)y * n + y]; });
    for (int j = 0; j < n; ++j) {
        w[j] = m[(size_t)order[j] * n + order[j]];
        for (int k = 0; k < n; ++k) v[(size_t)k * n + j] = u[(size_t)k * n + order[j]];
    }
    return done ? sweeps : -1;
}

namespace {

unsigned spectral_grid(const DiffuseWork* w, int64_t blocks) {
    return diffuse_grid(std::min<int64_t>(blocks, (int64_t)w->cus * DIF_BLOCKS_PER_CU));
}

using hclock = std::chrono::steady_clock;
double us_since(hclock::time_point t0) { return std::chrono::duration<double, std::micro>(hclock::now() - t0).count(); }

// The launches of a call on the work's stream.  timing ("diffuse_timing"): every launch sits between two events and the host waits
// for the second (family: 1 step, 2 gram with its tree, 3 rotate, 4 colnorm2 with its tree) -- the arithmetic is the same.
struct SpectralRun {
    DiffuseWork* w;
    const as_graph* gr;
    int64_t n;
    int C;
    bool timing;
    int64_t steps = 0, grams = 0, rotates = 0, waits = 0;

    double* pin_t() const { return w->spec_h; }                        // [C][C]: the matrix of the next rotate
    double* pin_theta() const { return pin_t() + C * C; }              // [C]
    double* pin_g() const { return pin_t() + C * C + C; }              // [C][C]: a Gram, downloaded
    double* pin_res() const { return pin_t() + 2 * C * C + C; }        // [C]: the squared residual norms, downloaded
    double* dev_t() const { return w->spec_d; }
    double* dev_theta() const { return dev_t() + C * C; }

    as_status reserve() {
        for (int s = 0; s < 2; ++s) {
            AS_TRY(reserve_or_err(w->f[s], n * C, "diffuse f buffers"));
            AS_TRY(reserve_or_err(w->sv[s], n * C, "diffuse solve vectors"));
        }
        const int64_t gseg = (n + SPC_GRAM_SEG - 1) / SPC_GRAM_SEG, dseg = (n + SPC_DOT_SEG - 1) / SPC_DOT_SEG;
        AS_TRY(reserve_or_err(w->part, std::max<int64_t>(gseg * C * C, dseg * C), "spectral partials"));
        AS_TRY(reserve_or_err(w->spec_d, C * C + C, "spectral matrix"));
        AS_TRY(reserve_or_err(w->spec_h, 2 * (C * C + C), "spectral pinned matrices"));
        if (timing && !w->spec_ev.e[0]) AS_HIP(w->spec_ev.create());
        return AS_OK;
    }
    as_status before() {
        if (timing) AS_HIP(hipEventRecord(w->spec_ev.e[0], w->stream));
        return AS_OK;
    }
    as_status after(int family) {
        AS_HIP(hipGetLastError());
        if (!timing) return AS_OK;
        AS_HIP(hipEventRecord(w->spec_ev.e[1], w->stream));
        AS_HIP(hipEventSynchronize(w->spec_ev.e[1]));
        float ms = 0.0f;
        AS_HIP(hipEventElapsedTime(&ms, w->spec_ev.e[0], w->spec_ev.e[1]));
        w->spectral_us[family] += (double)ms * 1e3;
        return AS_OK;
    }
    as_status wait() {
        const hclock::time_point t0 = hclock::now();
        AS_HIP(hipStreamSynchronize(w->stream));
        w->spectral_us[6] += us_since(t0);
        ++waits;
        return AS_OK;
    }

    as_status step(const double* v, const double* wv, double* out, double a, double b, double g) {
        SpectralStepArgs sa;
        sa.indptr = gr->indptr; sa.indices = gr->indices; sa.lap = gr->lap; sa.v = v; sa.w = wv; sa.out = out; sa.n = n;
        sa.a = a; sa.b = b; sa.g = g;
        const int64_t per_block = (int64_t)(DIF_THREADS / 64) * (64 / C);   // rows of a block and trip
        const unsigned grid = spectral_grid(w, (n + per_block - 1) / per_block);
        AS_TRY(before());
        if (C == 16) hipLaunchKernelGGL(spectral_step_kernel<16>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, sa);
        else hipLaunchKernelGGL(spectral_step_kernel<64>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, sa);
        ++steps;
        return after(1);
    }
    // G = A^T B into pin_g(); waits
    as_status gram(const double* A, const double* B) {
        const int64_t nseg = (n + SPC_GRAM_SEG - 1) / SPC_GRAM_SEG;
        const unsigned grid = spectral_grid(w, nseg);
        double* part = w->part;
        AS_TRY(before());
        if (C == 16) hipLaunchKernelGGL(spectral_gram_kernel<16>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, A, B, n, part);
        else hipLaunchKernelGGL(spectral_gram_kernel<64>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, A, B, n, part);
        hipLaunchKernelGGL(spectral_tree_kernel, dim3((unsigned)(C * C / 64)), dim3(SPC_TREE_THREADS), 0, w->stream, part, nseg, C * C, 64);
        ++grams;
        AS_TRY(after(2));
        AS_HIP(hipMemcpyAsync(pin_g(), part, sizeof(double) * (size_t)(C * C), hipMemcpyDeviceToHost, w->stream));
        return wait();
    }
    // the matrix in pin_t() (and, theta set, the values in pin_theta()) to the device: the host has waited since the last upload
    as_status upload(bool theta) {
        AS_HIP(hipMemcpyAsync(dev_t(), pin_t(), sizeof(double) * (size_t)(C * C + (theta ? C : 0)), hipMemcpyHostToDevice, w->stream));
        return AS_OK;
    }
    as_status rotate(const double* X, double* out) {
        const int64_t tile = (int64_t)(DIF_THREADS / C) * SPC_ROT_RPT;
        const unsigned grid = spectral_grid(w, (n + tile - 1) / tile);
        const size_t lds = sizeof(double) * (size_t)(C * C + tile * C);
        AS_TRY(before());
        if (C == 16) hipLaunchKernelGGL(spectral_rotate_kernel<16>, dim3(grid), dim3(DIF_THREADS), lds, w->stream, X, (const double*)dev_t(), n, out);
        else hipLaunchKernelGGL(spectral_rotate_kernel<64>, dim3(grid), dim3(DIF_THREADS), lds, w->stream, X, (const double*)dev_t(), n, out);
        ++rotates;
        return after(3);
    }
    // the squared column norms of Y - X theta (theta on the device) into pin_res(); waits
    as_status colnorm2(const double* X, const double* Y) {
        const int64_t nseg = (n + SPC_DOT_SEG - 1) / SPC_DOT_SEG;
        const int64_t per_block = (int64_t)(DIF_THREADS / 64) * (64 / C);   // segments of a block and trip
        const unsigned grid = spectral_grid(w, (nseg + per_block - 1) / per_block);
        double* part = w->part;
        AS_TRY(before());
        if (C == 16) hipLaunchKernelGGL(spectral_colnorm_kernel<16>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, X, Y, (const double*)dev_theta(), n, part);
        else hipLaunchKernelGGL(spectral_colnorm_kernel<64>, dim3(grid), dim3(DIF_THREADS), 0, w->stream, X, Y, (const double*)dev_theta(), n, part);
        hipLaunchKernelGGL(spectral_tree_kernel, dim3((unsigned)(C / 4)), dim3(SPC_TREE_THREADS), 0, w->stream, part, nseg, C, 4);
        AS_TRY(after(4));
        AS_HIP(hipMemcpyAsync(pin_res(), part, sizeof(double) * (size_t)C, hipMemcpyDeviceToHost, w->stream));
        return wait();
    }
    // x <- x (U Lambda^-1/2) of x^T x = U Lambda U^T, into `out`; *lost: an eigenvalue <= 1e-14 Lambda_max (nothing rotated)
    as_status orthonormalise(const double* x, double* out, bool* lost) {
        AS_TRY(gram(x, x));
        const hclock::time_point t0 = hclock::now();
        std::vector<double> lam(C), U((size_t)C * C);
        (void)sym_eig_host(pin_g(), C, lam.data(), U.data());
        w->spectral_us[5] += us_since(t0);
        *lost = !(lam[0] > SPC_BREAKDOWN * lam[C - 1]);   // (ascending; a NaN is a breakdown)
        if (*lost) return AS_OK;
        double* T = pin_t();
        for (int k = 0; k < C; ++k)
            for (int j = 0; j < C; ++j) T[k * C + j] = U[(size_t)k * C + j] / std::sqrt(lam[j]);
        AS_TRY(upload(false));
        return rotate(x, out);
    }
};

}  // namespace

static as_status spectral_eigs_run(const as_space* sp, const as_graph* gr, const SpectralCall& c, int64_t* counts) {
    const int64_t n = gr->n;
    const int C = c.C, m = c.m;
    DiffuseWork* w = nullptr;
    AS_TRY(diffuse_work_get(sp, &w));
    SpectralRun run{w, gr, n, C, diffuse_timing()};
    for (double& v : w->spectral_us) v = 0.0;
    AS_TRY(run.reserve());
    const hclock::time_point call0 = hclock::now();
    double *x = w->f[0], *y = w->f[1], *x2 = w->sv[0], *y2 = w->sv[1];
    int state = 0;
    int64_t it = 0;
    std::vector<double> theta(C), H((size_t)C * C), lam(C), Q((size_t)C * C);
    const int64_t cells = n * C;
    hipLaunchKernelGGL(spectral_start_kernel, dim3(spectral_grid(w, (cells + DIF_THREADS - 1) / DIF_THREADS)), dim3(DIF_THREADS), 0, w->stream, x,
                       cells, (uint64_t)c.seed * 0xBF58476D1CE4E5B9ull);
    AS_HIP(hipGetLastError());
    auto ortho_twice = [&](double*& blk, double*& spare) -> as_status {
        for (int pass = 0; pass < 2 && state != 2; ++pass) {
            bool lost = false;
            AS_TRY(run.orthonormalise(blk, spare, &lost));
            if (lost) state = 2;
            else std::swap(blk, spare);
        }
        return AS_OK;
    };
    AS_TRY(ortho_twice(x, y));
    while (state == 0) {
        ++it;
        // Rayleigh-Ritz: Y = S X, H = X^T Y, X <- X Q, Y <- Y Q, the residuals
        AS_TRY(run.step(x, nullptr, y, 1.0, 0.0, 0.0));
        AS_TRY(run.gram(x, y));
        const hclock::time_point t0 = hclock::now();
        const double* G = run.pin_g();
        for (int i = 0; i < C; ++i)
            for (int j = 0; j < C; ++j) H[(size_t)i * C + j] = 0.5 * (G[i * C + j] + G[j * C + i]);
        (void)sym_eig_host(H.data(), C, lam.data(), Q.data());
        double* T = run.pin_t();
        double* th = run.pin_theta();
        for (int j = 0; j < C; ++j) {   // descending
            theta[j] = th[j] = lam[C - 1 - j];
            for (int k = 0; k < C; ++k) T[k * C + j] = Q[(size_t)k * C + (C - 1 - j)];
        }
        w->spectral_us[5] += us_since(t0);
        AS_TRY(run.upload(true));
        AS_TRY(run.rotate(x, x2));
        AS_TRY(run.rotate(y, y2));
        AS_TRY(run.colnorm2(x2, y2));
        const double* r2 = run.pin_res();
        bool conv = true;
        for (int j = 0; j < m; ++j) {
            c.out_residuals[j] = std::sqrt(r2[j]);
            conv = conv && c.out_residuals[j] <= c.tol;
        }
        std::swap(x, x2);   // the Ritz vectors are the iterate; y and y2 and the old x are free
        if (conv) state = 1;
        if (conv || it >= c.max_iters) break;
        // the filter: Chebyshev over [lo, cut], the Ritz values steer it
        const double t1 = theta[0];
        double cut = std::min(theta[C - 1], t1 - SPC_GAP_FLOOR * (t1 - SPC_LO));
        cut = std::max(cut, SPC_LO + SPC_GAP_FLOOR * (t1 - SPC_LO));   // (a Ritz value at lo itself: the interval keeps a width)
        const double e = (cut - SPC_LO) / 2.0, ce = (cut + SPC_LO) / 2.0;
        const double tt = (t1 - ce) / e;
        const double dd = std::floor(std::log(SPC_GROWTH) / std::acosh(tt));
        const int d = std::max(1, (int)std::min((double)c.degree, dd));   // (dd NaN or huge: the min picks degree)
        double *zp = x, *z = y;
        AS_TRY(run.step(x, nullptr, z, 1.0 / e, -ce / e, 0.0));
        for (int j = 1; j < d; ++j) {
            AS_TRY(run.step(z, zp, zp, 2.0 / e, -2.0 * ce / e, -1.0));   // Z_{j+1} over Z_{j-1}'s block
            std::swap(z, zp);
        }
        // the filtered block is z and zp is free: the pair serves as the next x and y (x2 and y2 were not touched)
        x = z;
        y = zp;
        AS_TRY(ortho_twice(x, y));
    }
    if (state != 2) {
        for (int j = 0; j < m; ++j) c.out_values[j] = theta[j];
        // the answer's rows: [m][n] through a free block
        AS_TRY(reserve_or_err(w->rows, (int64_t)m * n, "spectral rows"));
        hipLaunchKernelGGL(spectral_rows_kernel, dim3(spectral_grid(w, (n + DIF_THREADS - 1) / DIF_THREADS)), dim3(DIF_THREADS), 0, w->stream,
                           (const double*)x, C, m, n, (double*)w->rows);
        AS_HIP(hipGetLastError());
        AS_HIP(hipMemcpyAsync(c.out_vectors, w->rows, sizeof(double) * (size_t)((int64_t)m * n), hipMemcpyDeviceToHost, w->stream));
        AS_TRY(run.wait());
        // the sign rule: the entry of largest magnitude, lowest index on ties, is positive
        for (int j = 0; j < m; ++j) {
            double* v = c.out_vectors + (int64_t)j * n;
            int64_t best = 0;
            for (int64_t i = 1; i < n; ++i)
                if (std::fabs(v[i]) > std::fabs(v[best])) best = i;
            if (v[best] < 0.0)
                for (int64_t i = 0; i < n; ++i) v[i] = -v[i];
        }
    }
    w->spectral_us[0] = us_since(call0);
    c.out_info[0] = it;
    c.out_info[1] = state;
    c.out_info[2] = run.steps;
    c.out_info[3] = C;
    counts[0] += it;
    counts[1] += run.steps;
    counts[2] += run.grams;
    counts[3] += run.rotates;
    counts[4] += run.waits;
    return AS_OK;
}

// the debug entry: host blocks up, exactly the launch the driver makes, the result down
static as_status spectral_op_run(const as_space* sp, const as_graph* gr, int op, int64_t n, int C, const double* a_host, const double* b_host,
                      const double* t_host, const double* coef, double* out_host) {
    DiffuseWork* w = nullptr;
    AS_TRY(diffuse_work_get(sp, &w));
    SpectralRun run{w, gr, n, C, false};
    AS_TRY(run.reserve());
    const size_t bytes = sizeof(double) * (size_t)(n * C);
    double *A = w->f[0], *B = w->f[1], *O = w->sv[0];
    AS_HIP(hipMemcpyAsync(A, a_host, bytes, hipMemcpyHostToDevice, w->stream));
    if (b_host) AS_HIP(hipMemcpyAsync(B, b_host, bytes, hipMemcpyHostToDevice, w->stream));
    if (op == AS_SPECTRAL_STEP) {
        double* out = coef[3] != 0.0 ? B : O;   // coef[3]: `out` is W's block
        AS_TRY(run.step(A, b_host ? B : nullptr, out, coef[0], coef[1], coef[2]));
        AS_HIP(hipMemcpyAsync(out_host, out, bytes, hipMemcpyDeviceToHost, w->stream));
        return run.wait();
    }
    if (op == AS_SPECTRAL_GRAM) {
        AS_TRY(run.gram(A, b_host ? B : A));
        std::memcpy(out_host, run.pin_g(), sizeof(double) * (size_t)(C * C));
        return AS_OK;
    }
    if (op == AS_SPECTRAL_ROTATE) {
        AS_HIP(hipStreamSynchronize(w->stream));   // (the pinned matrix of an earlier call is no longer read)
        std::memcpy(run.pin_t(), t_host, sizeof(double) * (size_t)(C * C));
        AS_TRY(run.upload(false));
        AS_TRY(run.rotate(A, O));
        AS_HIP(hipMemcpyAsync(out_host, O, bytes, hipMemcpyDeviceToHost, w->stream));
        return run.wait();
    }
    AS_HIP(hipStreamSynchronize(w->stream));
    std::memcpy(run.pin_theta(), t_host, sizeof(double) * (size_t)C);
    AS_TRY(run.upload(true));   // (the matrix ahead of theta travels with it and is not read)
    AS_TRY(run.colnorm2(A, B));
    std::memcpy(out_host, run.pin_res(), sizeof(double) * (size_t)C);
    return AS_OK;
}

// (a failed run leaves nothing on the stream when the caller releases the lock)
as_status spectral_eigs(const as_space* sp, const as_graph* gr, const SpectralCall& c, int64_t* counts) {
    const as_status s = spectral_eigs_run(sp, gr, c, counts);
    if (s != AS_OK && sp->diffuse_ws) (void)hipStreamSynchronize(sp->diffuse_ws->stream);
    return s;
}
as_status spectral_op(const as_space* sp, const as_graph* gr, int op, int64_t n, int C, const double* a_host, const double* b_host,
                      const double* t_host, const double* coef, double* out_host) {
    const as_status s = spectral_op_run(sp, gr, op, n, C, a_host, b_host, t_host, coef, out_host);
    if (s != AS_OK && sp->diffuse_ws) (void)hipStreamSynchronize(sp->diffuse_ws->stream);
    return s;
}

}  // namespace as
