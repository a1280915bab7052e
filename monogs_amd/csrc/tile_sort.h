// Per-tile depth sort (ForwardPlan::per_tile: large maps), shared by binning.hip (tile_depth_sort_kernel) and blend.hip
// (blend_forward_kernel<true>, which sorts its own tile before walking it).
//
// Instead of a global depth sort of all P Gaussians (three or four counted-tiles passes: ~105 us at C5, 2 M Gaussians),
// duplicate_kernel emits the instances in Gaussian-index order with the depth packed into the pair (see dup_pair), the
// stable tile sort groups them by tile -- index order inside a tile -- and ONE workgroup per tile sorts its list by depth
// here, stably, in LDS.  Result: (depth bits, index) order inside every tile, bit for bit what the two global sorts produce.
//   * a list of <= TDS_CAP pairs: keys = depth27 - (the tile's minimum), LSD passes of 9 bits over the significant bits
//     only (C5: 500 - 851 pairs per tile, ~25 significant bits: three passes).  Ranking as in the radix sort: a returning
//     LDS atomic on the wave's digit counter (lanes of one DS instruction in lane order, a wave's instructions in program
//     order: stable); wave w owns elements [w * 256, (w + 1) * 256), row i of them 64 consecutive ones.
//   * depths beyond the narrow range were clamped to DEPTH_KEY_NARROW: those pairs form the LAST run of the sorted list,
//     still in index order; it is re-sorted by the full depth key (gathered through the index), the same way.
//   * a longer list (a scene of large splats, never C5): the same LSD sort over the tile's segment in global memory,
//     256 pairs at a time with running digit offsets, on the full depth key, ping-ponging through the other half of the
//     tile sort's buffers (free once it is done); four 8-bit passes end in the original buffers.
// The indices are written in place over the tile's values: b.vals_sorted is the blend kernels' point_list.
#pragma once
#include "common.h"

namespace mgs {

constexpr int TDS_THREADS = 256, TDS_WAVES = TDS_THREADS / WAVE, TDS_ITEMS = 4, TDS_CAP = TDS_THREADS * TDS_ITEMS;
constexpr int TDS_DB = 9, TDS_RADIX = 1 << TDS_DB, TDS_DPT = TDS_RADIX / TDS_THREADS;

// LDS the sort works in: 4 KB of keys + 4 KB of values + 4 x 512 digit counters (8 KB) + 48 bytes of reductions
struct TdsLds {
    uint32_t* k;                               // [TDS_CAP]
    uint32_t* v;                               // [TDS_CAP]: the sorted indices once tile_depth_sort returns > 0
    uint32_t (*cnt)[TDS_RADIX];                // [TDS_WAVES]
    uint32_t* wsum;                            // [TDS_WAVES]
    uint32_t* red;                             // [2 * TDS_WAVES]
};

// block-wide min / max of one value per thread (valid lanes only); every thread gets both
__device__ __forceinline__ void tds_minmax(uint32_t lo, uint32_t hi, uint32_t* s_red /* >= 2 * TDS_WAVES */, uint32_t& mn,
                                           uint32_t& mx) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    MGS_WAVE_REDUCE2(lo, min, hi, max);
    if (lane == 0) { s_red[wv] = lo; s_red[TDS_WAVES + wv] = hi; }
    __syncthreads();
    mn = s_red[0]; mx = s_red[TDS_WAVES];
#pragma unroll
    for (int w = 1; w < TDS_WAVES; ++w) { mn = min(mn, s_red[w]); mx = max(mx, s_red[TDS_WAVES + w]); }
    __syncthreads();                                      // (s_red is reused)
}

// stable LSD sort of the LDS pairs [base, base + m), m <= TDS_CAP, on key bits [0, bits)
__device__ __forceinline__ void tds_lds_sort(uint32_t* s_k, uint32_t* s_v, uint32_t (*s_cnt)[TDS_RADIX], uint32_t* s_wsum,
                                             int base, int m, int bits) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int sh = 0; sh < bits; sh += TDS_DB) {
#pragma unroll
        for (int w = 0; w < TDS_WAVES; ++w)
#pragma unroll
            for (int j = 0; j < TDS_DPT; ++j) s_cnt[w][t * TDS_DPT + j] = 0u;
        __syncthreads();                                  // (also: the previous pass's scatter is visible)
        uint32_t k[TDS_ITEMS], v[TDS_ITEMS], r[TDS_ITEMS];
#pragma unroll
        for (int i = 0; i < TDS_ITEMS; ++i) {
            const int e = wv * (TDS_ITEMS * WAVE) + i * WAVE + lane;
            k[i] = 0u; v[i] = 0u; r[i] = 0u;
            if (e < m) {
                k[i] = s_k[base + e]; v[i] = s_v[base + e];
                r[i] = __hip_atomic_fetch_add(&s_cnt[wv][(k[i] >> sh) & (TDS_RADIX - 1)], 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        // thread t owns digits t * DPT + j: per-wave exclusive prefixes on top of the exclusive prefix over the digits
        uint32_t c[TDS_DPT][TDS_WAVES], tot[TDS_DPT], tsum = 0;
#pragma unroll
        for (int j = 0; j < TDS_DPT; ++j) {
            tot[j] = 0u;
#pragma unroll
            for (int w = 0; w < TDS_WAVES; ++w) { c[j][w] = s_cnt[w][t * TDS_DPT + j]; tot[j] += c[j][w]; }
            tsum += tot[j];
        }
        const uint32_t incl = wave_incl_scan_dpp(tsum);
        if (lane == 63) s_wsum[wv] = incl;
        __syncthreads();
        uint32_t run = incl - tsum;
        for (int w = 0; w < wv; ++w) run += s_wsum[w];
#pragma unroll
        for (int j = 0; j < TDS_DPT; ++j)
#pragma unroll
            for (int w = 0; w < TDS_WAVES; ++w) { s_cnt[w][t * TDS_DPT + j] = run; run += c[j][w]; }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TDS_ITEMS; ++i) {
            const int e = wv * (TDS_ITEMS * WAVE) + i * WAVE + lane;
            if (e < m) {
                const uint32_t dst = s_cnt[wv][(k[i] >> sh) & (TDS_RADIX - 1)] + r[i];
                s_k[base + dst] = k[i]; s_v[base + dst] = v[i];
            }
        }
        __syncthreads();                                  // (every wave is done with the offsets before the next pass clears them)
    }
    __syncthreads();
}

// A list longer than TDS_CAP: stable LSD sort of the segment [0, n) of (kx, vx) on the full depth key, 8 bits per pass,
// ping-ponging through (ky, vy); rare (large splats), so simple: one pair per thread per step.
__device__ inline void tds_global_sort(uint32_t* __restrict__ kx, uint32_t* __restrict__ vx, uint32_t* __restrict__ ky,
                                       uint32_t* __restrict__ vy, uint32_t n, const uint32_t* __restrict__ depth_key, int lo,
                                       uint32_t (*s_cnt)[TDS_RADIX], uint32_t* s_run, uint32_t* s_wsum) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t imask = lo ? (1u << (32 - lo)) - 1u : 0xFFFFFFFFu;
    for (uint32_t e = t; e < n; e += TDS_THREADS) {       // in place: (packed key, packed value) -> (full key, index)
        const uint32_t g = vx[e] & imask;
        kx[e] = depth_key[g] - DEPTH_KEY_SUB;
        vx[e] = g;
    }
    for (int sh = 0; sh < 32; sh += 8) {
        __threadfence();                                  // (this workgroup's stores, read back by other lanes)
        if (t < 256) s_run[t] = 0u;
#pragma unroll
        for (int w = 0; w < TDS_WAVES; ++w) s_cnt[w][t] = 0u;
        __syncthreads();
        for (uint32_t e = t; e < n; e += TDS_THREADS) atomicAdd(&s_run[(kx[e] >> sh) & 255u], 1u);
        __syncthreads();
        {                                                 // exclusive scan of the 256 digit counts: running offsets
            const uint32_t c = s_run[t], incl = wave_incl_scan_dpp(c);
            if (lane == 63) s_wsum[wv] = incl;
            __syncthreads();
            uint32_t b0 = incl - c;
            for (int w = 0; w < wv; ++w) b0 += s_wsum[w];
            s_run[t] = b0;
        }
        __syncthreads();
        for (uint32_t c0 = 0; c0 < n; c0 += TDS_THREADS) {
            const uint32_t e = c0 + (uint32_t)t;          // element order = (wave, lane) order
            uint32_t k = 0u, v = 0u, r = 0u, d = 0u;
            if (e < n) {
                k = kx[e]; v = vx[e]; d = (k >> sh) & 255u;
                r = __hip_atomic_fetch_add(&s_cnt[wv][d], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            __syncthreads();
            uint32_t pre[TDS_WAVES];                      // thread t = digit t: where each wave's pairs of it go
            {
                uint32_t run = s_run[t];
#pragma unroll
                for (int w = 0; w < TDS_WAVES; ++w) { const uint32_t c = s_cnt[w][t]; pre[w] = run; run += c; }
                s_run[t] = run;
            }
            __syncthreads();
#pragma unroll
            for (int w = 0; w < TDS_WAVES; ++w) s_cnt[w][t] = pre[w];
            __syncthreads();
            if (e < n) { const uint32_t dst = s_cnt[wv][d] + r; ky[dst] = k; vy[dst] = v; }
            __syncthreads();
#pragma unroll
            for (int w = 0; w < TDS_WAVES; ++w) s_cnt[w][t] = 0u;
            __syncthreads();
        }
        __threadfence();
        __syncthreads();
        uint32_t* tk = kx; kx = ky; ky = tk;
        uint32_t* tv = vx; vx = vy; vy = tv;
    }
}

// Sorts one tile's list (the tile sort's raw range `rg`: {first, last + 1}, or {~0, 0} when empty) by (depth bits, index)
// and writes the indices in place over ts.vals.  Called by all 256 threads of the tile's workgroup; every condition that
// skips work is uniform over the workgroup, so every barrier inside is reached by all four waves.  Nothing is sorted for
// an empty tile or when `skip` (the tile sort's look-back timed out: the ranges are invalid).  Returns n when the list
// (n <= TDS_CAP pairs) was sorted in LDS -- lds.v[0, n) then holds the sorted indices too, and lds.k / lds.cnt are free
// (the last barrier is behind their last use) -- else 0.  The global-memory writes are not waited for.
__device__ __forceinline__ uint32_t tile_depth_sort(const TileSortArgs& ts, uint2 rg, bool skip, const TdsLds& lds) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t n_live = ts.n_dev ? min(ts.n_cap, ts.n_dev[0]) : ts.n_cap;     // capacity mode: never past the live pairs
    const uint32_t start = rg.x, end = min(rg.y, n_live);
    if (skip || start >= end) return 0u;
    const uint32_t n = end - start;
    const int lo = tile_depth_lo_bits(ts.tb);
    const uint32_t kmask = ts.tb < 32 ? (0xFFFFFFFFu >> ts.tb) : 0u, imask = lo ? (1u << (32 - lo)) - 1u : 0xFFFFFFFFu;
    if (n > (uint32_t)TDS_CAP) {
        uint32_t* const k = ts.keys + start;
        uint32_t* const v = ts.vals + start;
        tds_global_sort(k, v, ts.keys_alt + start, ts.vals_alt + start, n, ts.depth_key, lo, lds.cnt, lds.k, lds.wsum);
        return 0u;
    }
    // ---- load (wave-striped), unpack depth27 and index, range of the depths
    uint32_t d[TDS_ITEMS], g[TDS_ITEMS];
    uint32_t dmin = 0xFFFFFFFFu, dmax = 0u;
#pragma unroll
    for (int i = 0; i < TDS_ITEMS; ++i) {
        const uint32_t e = (uint32_t)(wv * (TDS_ITEMS * WAVE) + i * WAVE + lane);
        d[i] = 0u; g[i] = 0u;
        if (e < n) {
            const uint32_t k = ts.keys[start + e], v = ts.vals[start + e];
            d[i] = ((k & kmask) << lo) | (lo ? v >> (32 - lo) : 0u);
            g[i] = v & imask;
            dmin = min(dmin, d[i]); dmax = max(dmax, d[i]);
        }
    }
    uint32_t mn, mx;
    tds_minmax(dmin, dmax, lds.red, mn, mx);
#pragma unroll
    for (int i = 0; i < TDS_ITEMS; ++i) {
        const int e = wv * (TDS_ITEMS * WAVE) + i * WAVE + lane;
        if (e < (int)n) { lds.k[e] = d[i] - mn; lds.v[e] = g[i]; }
    }
    const uint32_t span = mx - mn;
    tds_lds_sort(lds.k, lds.v, lds.cnt, lds.wsum, 0, (int)n, span ? 32 - __builtin_clz(span) : 0);
    if (mx == DEPTH_KEY_NARROW) {
        // ---- clamped depths: the trailing run of keys DEPTH_KEY_NARROW - mn, in index order; re-sort it by the full key
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < TDS_ITEMS; ++i) {
            const uint32_t e = (uint32_t)(wv * (TDS_ITEMS * WAVE) + i * WAVE + lane);
            c += (e < n && d[i] == DEPTH_KEY_NARROW) ? 1u : 0u;
        }
        MGS_WAVE_REDUCE(c, MGS_WAVE_ADD);
        if (lane == 0) lds.red[wv] = c;
        __syncthreads();
        uint32_t m = 0;
#pragma unroll
        for (int w = 0; w < TDS_WAVES; ++w) m += lds.red[w];
        __syncthreads();
        const uint32_t f = n - m;                                    // first pair of the run
        uint32_t xmin = 0xFFFFFFFFu, xmax = 0u;
        for (uint32_t e = f + t; e < n; e += TDS_THREADS) {
            const uint32_t x = ts.depth_key[lds.v[e]] - DEPTH_KEY_SUB;
            lds.k[e] = x;
            xmin = min(xmin, x); xmax = max(xmax, x);
        }
        uint32_t rmn, rmx;
        tds_minmax(xmin, xmax, lds.red, rmn, rmx);
        for (uint32_t e = f + t; e < n; e += TDS_THREADS) lds.k[e] -= rmn;
        __syncthreads();
        const uint32_t rspan = rmx - rmn;
        tds_lds_sort(lds.k, lds.v, lds.cnt, lds.wsum, (int)f, (int)m, rspan ? 32 - __builtin_clz(rspan) : 0);
    }
    // ---- the indices, in place (coalesced)
#pragma unroll
    for (int i = 0; i < TDS_ITEMS; ++i) {
        const int e = wv * (TDS_ITEMS * WAVE) + i * WAVE + lane;
        if (e < (int)n) ts.vals[start + e] = lds.v[e];
    }
    return n;
}

}  // namespace mgs
