// The four-row gather trip of the filtered score kernels: the one dot-product body behind
// subset_score_kernel (as_subset.hip), lists_score_kernel (as_lists.hip) and diverse_select_kernel (as_diverse.hip).
// The rule for a change here: results stay bit-identical, every instantiation of the three callers keeps its occupancy class
// (at most 128 VGPRs: 4 waves per SIMD) and stays free of scratch, and the measured kernel times match the parent commit's.
#pragma once
#include "as_common.hpp"

#if defined(__HIPCC__)
namespace as {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int GATHER_ROWS = 4;       // rows in flight per wave: every load of the four is issued before the first FMA
constexpr int GATHER_Q_LDS = 4096;   // the query sits in LDS up to this many doubles (32 KiB a block); longer ones are read from global memory
static_assert(GATHER_ROWS == 4, "the callers' lane selects (row and sum of lane 0 .. 3) are written for four rows");

// acc[r] = the lane's share of <query, row[r]>, r < GATHER_ROWS; the caller's wave_sum butterfly makes the dot products of it.
// One wave, the row ids wave-uniform.  F64: the rows are the fp64 items ([n][d], rows 8-byte aligned: one double per lane and
// load); else the fp32 items ([np][dp], zero padded, dp a multiple of 32: 16 bytes per lane and load), widened before the
// product.  QLDS: query element e is qs[e] (LDS, staged by the caller); else qg(e), the caller's read of it from global memory.
// Element e of a row is always lane (e % 64) (fp64) or lane (e / 4 % 64) (fp32), and a lane adds its products in ascending e,
// one `acc[r] += qv * v` each: the bits of a dot product depend on the query and the row alone.
template <bool F64, bool QLDS, class QG>
__device__ __forceinline__ void gather_trip(const float* x32, const double* x64, int64_t d, int64_t dp, const int64_t (&row)[GATHER_ROWS],
                                            const double* qs, QG qg, int lane, double (&acc)[GATHER_ROWS]) {
#pragma unroll
    for (int r = 0; r < GATHER_ROWS; ++r) acc[r] = 0.0;
    if (F64) {
        constexpr int U = 6;   // 64 doubles per load of a wave: 384 columns of 4 rows before the first FMA
        for (int64_t base = 0; base < d; base += 64 * U) {
            double v[GATHER_ROWS][U];
#pragma unroll
            for (int r = 0; r < GATHER_ROWS; ++r) {
                const double* pj = x64 + row[r] * d;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t e = base + 64 * u + lane;
                    v[r][u] = e < d ? pj[e] : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t e = base + 64 * u + lane;
                if (e < d) {
                    const double qv = QLDS ? qs[e] : qg(e);
#pragma unroll
                    for (int r = 0; r < GATHER_ROWS; ++r) acc[r] += qv * v[r][u];
                }
            }
        }
    } else {
        constexpr int U = 3;   // 256 floats per load of a wave: a whole 768-float row of 4 rows before the first FMA
        for (int64_t base = 0; base < dp; base += 256 * U) {
            f32x4 v[GATHER_ROWS][U];
#pragma unroll
            for (int r = 0; r < GATHER_ROWS; ++r) {
                const float* pj = x32 + row[r] * dp;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t e = base + 256 * u + 4 * lane;   // (dp is a multiple of 32: e < dp leaves 4 floats)
                    v[r][u] = e < dp ? *(const f32x4*)(pj + e) : f32x4{0, 0, 0, 0};
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t e = base + 256 * u + 4 * lane;
                if (e < dp) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const double qv = QLDS ? qs[e + t] : qg(e + t);
#pragma unroll
                        for (int r = 0; r < GATHER_ROWS; ++r) acc[r] += qv * (double)v[r][u][t];
                    }
                }
            }
        }
    }
}

}  // namespace as
#endif
