// Range search: every item of a subset whose S11 score reaches a threshold, however many there are.
// The scores come from the filtered forms' score kernels (as_subset.hip), unchanged; this file turns a [nq][ld] block of them
// into only the survivors (range_compact_kernel: ballot ranks, one returning atomic per block on one slot counter, 16-byte
// entries in one append buffer) and, on the host, into each query's list by (score descending, id ascending).
// Entry points: as_api.hip (as_search_range, as_search_range_batch, the as_range accessors).
#include <algorithm>
#include <atomic>
#include <limits>
#include <new>

#include "as_common.hpp"

namespace as {

typedef double f64x2 __attribute__((ext_vector_type(2)));

struct RangeEntry {
    int32_t q;     // row of the block (the query's number inside its chunk)
    int32_t pos;   // position in the subset's sorted id list
    double score;
};
static_assert(sizeof(RangeEntry) == 16, "one 16-byte store per survivor");

constexpr int RC_THREADS = 256;
constexpr int RC_PAIRS = 4;                               // 16-byte loads per thread and trip
constexpr int RC_TRIP = RC_THREADS * RC_PAIRS * 2;        // scores per block and trip: 2048
constexpr int RC_BLOCKS = 2048;                           // blocks per launch, over all rows (the rest is the grid-stride loop)

// Row blockIdx.y of the scores against thr[blockIdx.y] (s >= thr in fp64: a NaN score, and any score against a NaN threshold,
// fails).  A row starts on an 8-byte boundary only (ld may be odd): the trip's windows are laid over `virtual` positions v = i +
// head, head = 1 where the row starts in the upper half of a 16-byte line, so that an even v is a 16-byte aligned address; every
// lane loads one aligned pair per window, the pair that straddles an end of the row as single doubles.  Per trip: a ballot per
// element slot gives the wave's survivor count and each survivor's rank inside the wave; the four counts meet in LDS; thread 0
// draws the block's slots with one returning atomicAdd on cnt[0] (only if the block has a survivor); a survivor is stored when
// its slot is below cap, so cnt[0] ends as the exact total whatever cap is.  COUNT: nothing is stored and no slot is drawn: the
// block's survivors over all its trips go to the row's own counter cnt[1 + row] with one atomic at the end.
template <bool COUNT>
__global__ __launch_bounds__(RC_THREADS) void range_compact_kernel(const double* __restrict__ scores, int64_t ld, int64_t m,
                                                                   const double* __restrict__ thr, RangeEntry* __restrict__ buf,
                                                                   unsigned long long cap, unsigned long long* __restrict__ cnt) {
    __shared__ unsigned int wcnt[2][RC_THREADS / 64];
    __shared__ unsigned long long base[2];
    const int q = blockIdx.y;
    const double t = thr[q];
    const double* row = scores + (int64_t)q * ld;
    const int64_t head = (int64_t)(((uintptr_t)row >> 3) & 1);
    const int64_t mv = m + head;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;   // the lanes in front of this one
    const double nan = __builtin_nan("");
    unsigned int kept = 0;   // COUNT: the wave's survivors so far
    int par = 0;
    for (int64_t b0 = (int64_t)blockIdx.x * RC_TRIP; b0 < mv; b0 += (int64_t)gridDim.x * RC_TRIP, par ^= 1) {
        double s[2 * RC_PAIRS];
        int64_t at[RC_PAIRS];
#pragma unroll
        for (int j = 0; j < RC_PAIRS; ++j) {
            const int64_t i0 = b0 + 2 * ((int64_t)threadIdx.x + RC_THREADS * j) - head, i1 = i0 + 1;
            at[j] = i0;
            const bool a0 = i0 >= 0 && i0 < m, a1 = i1 < m;
            if (a0 && a1) {
                const f64x2 x = *(const f64x2*)(row + i0);
                s[2 * j] = x[0];
                s[2 * j + 1] = x[1];
            } else {
                s[2 * j] = a0 ? row[i0] : nan;
                s[2 * j + 1] = a1 ? row[i1] : nan;
            }
        }
        unsigned int rank[2 * RC_PAIRS], wtot = 0;
#pragma unroll
        for (int e = 0; e < 2 * RC_PAIRS; ++e) {
            const unsigned long long mask = __ballot(s[e] >= t);
            rank[e] = wtot + (unsigned int)__popcll(mask & below);
            wtot += (unsigned int)__popcll(mask);
        }
        if (COUNT) {
            kept += wtot;
            continue;
        }
        if (lane == 0) wcnt[par][w] = wtot;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int total = 0;
#pragma unroll
            for (int u = 0; u < RC_THREADS / 64; ++u) total += wcnt[par][u];
            if (total) base[par] = atomicAdd(cnt, (unsigned long long)total);
        }
        __syncthreads();   // (the next trip writes the other halves of wcnt and base)
        unsigned long long slot0 = base[par];
        for (int u = 0; u < w; ++u) slot0 += wcnt[par][u];
#pragma unroll
        for (int e = 0; e < 2 * RC_PAIRS; ++e) {
            const unsigned long long slot = slot0 + rank[e];
            if (s[e] >= t && slot < cap) {
                RangeEntry r;
                r.q = q;
                r.pos = (int32_t)(at[e >> 1] + (e & 1));
                r.score = s[e];
                buf[slot] = r;
            }
        }
    }
    if (COUNT) {
        if (lane == 0) wcnt[0][w] = kept;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int total = 0;
#pragma unroll
            for (int u = 0; u < RC_THREADS / 64; ++u) total += wcnt[0][u];
            if (total) atomicAdd(cnt + 1 + q, (unsigned long long)total);
        }
    }
}

// ------------------------------------------------------------------ host side
// Entries of the append buffer a call starts with: 65 536 (1 MiB) by default, or whatever earlier overflows grew the buffer to;
// as_set_tuning("range_cap", v > 0): exactly v, whatever the buffer holds.  Results never depend on it.
constexpr int64_t RANGE_CAP_DEFAULT = 65536;
constexpr int64_t RANGE_SPEC = 4096;   // entries copied to the host together with the counter, before the chunk's one wait
static std::atomic<int> g_range_cap{0};
static std::atomic<int> g_range_timing{0};
void set_range_cap(int v) { g_range_cap.store(v > 0 ? v : 0, std::memory_order_relaxed); }
void set_range_timing(int v) { g_range_timing.store(v ? 1 : 0, std::memory_order_relaxed); }

struct RangeWork {
    dev_buf<RangeEntry> buf;           // the append buffer
    dev_buf<unsigned long long> cnt;   // [1 + rows]: the slot counter, then one counter per row (count_only)
    dev_buf<double> thr;               // [rows]; rows: a power of two, at least 64
    pin_buf<unsigned long long> hcnt;  // pinned [1 + rows]
    pin_buf<double> hthr;              // pinned [rows]
    pin_buf<RangeEntry> hent;          // pinned: the front of the append buffer, or all of it
    dev_events<2> ev;                  // made by the first call under "range_timing"
};

void range_work_free(RangeWork* r) { delete r; }

as_status range_compact(SubsetWork* w, const double* scores, int64_t ld, int64_t m, int64_t nq, const double* thr_host, bool count_only,
                        const int64_t* ids_host, as_range* res, int64_t* counts, double* us) {
    if (nq <= 0) return AS_OK;
    if (!w->range) {
        w->range = new (std::nothrow) RangeWork();
        if (!w->range) {
            set_err("range: out of host memory");
            return AS_ENOMEM;
        }
    }
    RangeWork* r = w->range;
    const bool timing = g_range_timing.load(std::memory_order_relaxed) != 0;
    if (timing && !r->ev.e[1]) AS_HIP(r->ev.create());
    int64_t rows = 64;
    while (rows < nq) rows *= 2;
    AS_TRY(reserve_or_err(r->cnt, rows + 1, "range counters"));
    AS_TRY(reserve_or_err(r->thr, rows, "range thresholds"));
    AS_TRY(reserve_or_err(r->hcnt, rows + 1, "range pinned counters"));
    AS_TRY(reserve_or_err(r->hthr, rows, "range pinned thresholds"));
    const int64_t tuned = g_range_cap.load(std::memory_order_relaxed);
    int64_t cap = 0;
    if (!count_only) {
        cap = tuned > 0 ? tuned : std::max<int64_t>(RANGE_CAP_DEFAULT, (int64_t)r->buf.size());
        AS_TRY(reserve_or_err(r->buf, cap, "range append buffer"));
        AS_TRY(reserve_or_err(r->hent, std::min<int64_t>(cap, RANGE_SPEC), "range pinned entries"));
    }
    int64_t live = 0;
    for (int64_t t = 0; t < nq; ++t) {
        r->hthr[t] = thr_host[t];
        live += thr_host[t] == thr_host[t] ? 1 : 0;
    }
    AS_HIP(hipMemcpyAsync(r->thr, r->hthr, sizeof(double) * (size_t)nq, hipMemcpyHostToDevice, w->stream));
    const int64_t trips = (m + 1 + RC_TRIP - 1) / RC_TRIP;
    const dim3 grid((unsigned)filtered_grid(std::max<int64_t>(1, std::min<int64_t>(trips, std::max<int64_t>(1, RC_BLOCKS / nq)))), (unsigned)nq);
    const size_t cnt_bytes = sizeof(unsigned long long) * (size_t)(count_only ? nq + 1 : 1);
    auto launch = [&](int64_t c) -> as_status {
        RangeEntry* buf = r->buf;
        unsigned long long* cnt = r->cnt;
        AS_HIP(hipMemsetAsync(cnt, 0, cnt_bytes, w->stream));
        if (timing) AS_HIP(hipEventRecord(r->ev.e[0], w->stream));
        if (count_only)
            hipLaunchKernelGGL(range_compact_kernel<true>, grid, dim3(RC_THREADS), 0, w->stream, scores, ld, m, (const double*)r->thr, buf, 0ull, cnt);
        else
            hipLaunchKernelGGL(range_compact_kernel<false>, grid, dim3(RC_THREADS), 0, w->stream, scores, ld, m, (const double*)r->thr, buf,
                               (unsigned long long)c, cnt);
        AS_HIP(hipGetLastError());
        if (timing) AS_HIP(hipEventRecord(r->ev.e[1], w->stream));
        AS_HIP(hipMemcpyAsync(r->hcnt, cnt, cnt_bytes, hipMemcpyDeviceToHost, w->stream));
        counts[0] += 1;
        return AS_OK;
    };
    auto wait = [&]() -> as_status { return sync_add_elapsed(w->stream, timing, r->ev.e, us); };
    AS_TRY(launch(cap));
    int64_t have = 0;   // entries of the buffer's front already on the host
    if (!count_only) {
        have = std::min<int64_t>(cap, RANGE_SPEC);
        AS_HIP(hipMemcpyAsync(r->hent, r->buf, sizeof(RangeEntry) * (size_t)have, hipMemcpyDeviceToHost, w->stream));
    }
    AS_TRY(wait());
    counts[1] += live * m;
    try {
        if (count_only) {
            for (int64_t t = 0; t < nq; ++t) {
                res->offs.push_back(res->offs.back() + (int64_t)r->hcnt[1 + t]);
                counts[2] += (int64_t)r->hcnt[1 + t];
            }
            res->nq += nq;
            return AS_OK;
        }
        const int64_t total = (int64_t)r->hcnt[0];
        if (total > cap) {
            // the scores are still in their buffer: only the compaction runs again, into a buffer that holds them all
            AS_TRY(reserve_or_err(r->buf, std::max<int64_t>(total, std::min<int64_t>(2 * cap, (int64_t)1 << 24)), "range append buffer"));
            AS_TRY(launch((int64_t)r->buf.size()));
            counts[3] += 1;
            have = 0;
            AS_TRY(wait());
            if ((int64_t)r->hcnt[0] != total) {
                set_err("range: the compaction counted %lld survivors, then %lld", (long long)total, (long long)r->hcnt[0]);
                return AS_EHIP;
            }
        }
        if (total > have) {
            AS_TRY(reserve_or_err(r->hent, total, "range pinned entries"));   // (a larger block: the front is copied again with the rest)
            AS_HIP(hipMemcpyAsync(r->hent, r->buf, sizeof(RangeEntry) * (size_t)total, hipMemcpyDeviceToHost, w->stream));
            AS_HIP(hipStreamSynchronize(w->stream));
        }
        // the entries by row (a counting sort: arrival order inside a row), ids for positions, then each row's own order
        std::vector<int64_t> start((size_t)nq + 1, 0);
        for (int64_t e = 0; e < total; ++e) {
            const RangeEntry& x = r->hent[e];
            if (x.q < 0 || x.q >= nq || x.pos < 0 || x.pos >= m) {
                set_err("range: entry %lld of the append buffer is out of range (row %d, position %d)", (long long)e, x.q, x.pos);
                return AS_EHIP;
            }
            start[(size_t)x.q + 1] += 1;
        }
        for (int64_t t = 0; t < nq; ++t) start[(size_t)t + 1] += start[(size_t)t];
        struct Hit {
            int64_t id;
            double score;
        };
        std::vector<Hit> hits((size_t)total);
        std::vector<int64_t> fill(start.begin(), start.end() - 1);
        for (int64_t e = 0; e < total; ++e) {
            const RangeEntry& x = r->hent[e];
            hits[(size_t)fill[(size_t)x.q]++] = Hit{ids_host ? ids_host[x.pos] : (int64_t)x.pos, x.score};
        }
        const int64_t at = res->offs.back();
        res->idx.resize((size_t)(at + total));
        res->score.resize((size_t)(at + total));
        for (int64_t t = 0; t < nq; ++t) {
            std::sort(hits.begin() + start[(size_t)t], hits.begin() + start[(size_t)t + 1],
                      [](const Hit& a, const Hit& b) { return a.score > b.score || (a.score == b.score && a.id < b.id); });
            res->offs.push_back(at + start[(size_t)t + 1]);
        }
        for (int64_t e = 0; e < total; ++e) {
            res->idx[(size_t)(at + e)] = hits[(size_t)e].id;
            res->score[(size_t)(at + e)] = hits[(size_t)e].score;
        }
        res->nq += nq;
        counts[2] += total;
    } catch (const std::bad_alloc&) {
        set_err("range: out of host memory for the answer");
        return AS_ENOMEM;
    }
    return AS_OK;
}

}  // namespace as
