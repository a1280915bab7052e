// Diagnostics of the blend walks: kernels the product never launches on its own, kept out of blend.hip.
//   mgs_debug_blend_stats        blend_backward_stats_kernel + blend_group_stats_kernel: what the backward walk does, counted
//   mgs_debug_blend_mask_stats   blend_mask_stats_kernel: the forward's survivor masks against the backward's own cull
//   mgs_debug_valu_ceiling       valu_ceiling_kernel: the plain-FMA issue ceiling of the chip
// The three counting kernels walk a quadrant's list as blend_backward_kernel does (tile_walk.h: the quadrant, the cull, the
// falloff and the activity rule), with counters instead of gradient arithmetic.
#include "common.h"
#include "tile_walk.h"

namespace mgs {

// ---- diagnostic: what the backward walk does, counted (not on the hot path; mgs_debug_blend_stats) --------------
// The same walk, cull and per-pixel activity test as blend_backward_kernel<1, *>, with counters instead of gradient
// arithmetic: stats[0] steps of 64 instances, [1] instances that pass the quadrant cull and are fetched ("survivors"),
// [2] survivors with at least one active pixel ("active survivors" = wave reductions = atomic instructions),
// [3] active (pixel, instance) pairs, [4] inactive survivors whose cull box holds no pixel with k <= last (depth
// order, not geometry), [5..7] active survivors with <= 2 / <= 4 / <= 8 active pixels.
__global__ void __launch_bounds__(256) blend_backward_stats_kernel(BlendArgs a, int ntiles,
                                                                   const uint32_t* __restrict__ n_contrib,
                                                                   unsigned long long* __restrict__ stats) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x;
    if (tile >= ntiles) return;
    const uint2 range = a.ranges[tile];
    if (range.y <= range.x) return;
    Quadrant q;
    MGS_QUADRANT_FILL(q, a, tile, wave, lane);
    const float qx0 = q.qx0(), qy0 = q.qy0();
    const uint32_t last = q.inside ? n_contrib[q.pix] : 0u;
    const uint32_t maxc = wave_max_u32(last);
    if (maxc == 0) return;
    const uint32_t end = range.x + maxc;
    unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = (int)((maxc - 1) / WAVE); b >= 0; --b) {
        const uint32_t i = range.x + (uint32_t)b * WAVE + lane;
        uint32_t gid_l = 0;
        float4 box = make_float4(0.f, 0.f, -1.f, -1.f), el = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < end) {
            gid_l = a.point_list[i];
            box = a.rec[(size_t)gid_l * 4];
            el = a.rec[(size_t)gid_l * 4 + 3];
        }
        const unsigned long long alive = __builtin_amdgcn_ballot_w64(last >= (uint32_t)b * WAVE + 1u);
        unsigned long long mask = __builtin_amdgcn_ballot_w64(quadrant_hit(box, el, qx0, qy0, alive));
        c[0] += 1;
        c[1] += __popcll(mask);
        while (mask) {
            const int j = 63 - __builtin_clzll(mask);
            mask &= ~(1ull << j);
            const uint32_t k = (uint32_t)b * WAVE + (uint32_t)j + 1u;
            const Rec g = fetch(reinterpret_cast<const float*>(a.rec), bcast(gid_l, j));
            const float dx = g.px - q.pxf, dy = g.py - q.pyf;
            const float power = falloff_power(dx, dy, g.ca, g.cb, g.cc);
            const float alpha = falloff_alpha(g.op, __builtin_amdgcn_exp2f(power));
            const bool geo = falloff_active(true, power, alpha);
            const unsigned long long act = __builtin_amdgcn_ballot_w64(geo && k <= last);
            const int n = __popcll(act);
            if (n == 0) {
                if (__builtin_amdgcn_ballot_w64(geo) != 0ull) c[4] += 1;
                continue;
            }
            c[2] += 1;
            c[3] += n;
            c[5] += n <= 2;
            c[6] += n <= 4;
            c[7] += n <= 8;
        }
    }
    if (lane < 8) {
        unsigned long long v = c[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) v = lane == k ? c[k] : v;
        atomicAdd(stats + lane, v);
    }
}

// ---- diagnostic, round 5: how many loop trips would the walk take if the wave ran SEVERAL survivor streams side by side,
// one per group of pixels?  39 of a survivor's 64 lanes are active on average (stats[3] / stats[2]) and narrowing EXEC saves
// no time on gfx950, so the only way to use the idle lanes is to give them another survivor.  For five ways of cutting the
// 8x8 quadrant into groups (two 8x4 halves, two 4x8 halves, four 4x4 blocks, four 8x2 strips, eight 4x2 blocks) the cull is
// run per group (the same box + ellipse test against the group's rectangle and its alive pixels) and three sums are kept:
//   [8 + 3 d + 0]  sum over steps of max_g S_g      trips when the groups' lists are paired step by step
//   [8 + 3 d + 1]  sum over steps of sum_g S_g      (group, survivor) rows: what the backward would have to flush
//   [8 + 3 d + 2]  sum over walks of max_g sum_steps S_g   trips when every group runs down a list of its own
// to be read against stats[1] (survivors of the whole-quadrant cull = trips now).
__device__ __forceinline__ bool rect_hit(const float4 c, const float4 n, float qx0, float qy0, int ox, int oy, int w, int h,
                                         unsigned long long alive) {
    if (c.z < 0.f) return false;
    const float x0q = qx0 - 0.05f - c.x, y0q = qy0 - 0.05f - c.y;                      // quadrant origin relative to the centre
    const float x0 = x0q + (float)ox, x1 = qx0 + (float)(ox + w - 1) + 0.05f - c.x;   // the group's rectangle
    const float y0 = y0q + (float)oy, y1 = qy0 + (float)(oy + h - 1) + 0.05f - c.y;
    if (!((c.z >= x0) && (-c.z <= x1) && (c.w >= y0) && (-c.w <= y1))) return false;
    {
        const int ix0 = (int)fminf(8.f, fmaxf(0.f, ceilf(-x0q - c.z - 0.06f))), ix1 = (int)fminf(7.f, fmaxf(-1.f, floorf(-x0q + c.z + 0.06f)));
        const int iy0 = (int)fminf(8.f, fmaxf(0.f, ceilf(-y0q - c.w - 0.06f))), iy1 = (int)fminf(7.f, fmaxf(-1.f, floorf(-y0q + c.w + 0.06f)));
        if (ix0 > ix1 || iy0 > iy1) return false;
        const unsigned long long cols = (unsigned long long)((0xFFu >> (7 - ix1)) & (0xFFu << ix0) & 0xFFu) * 0x0101010101010101ull;
        const unsigned long long rows = (~0ull >> (8 * (7 - iy1))) & (~0ull << (8 * iy0));
        const unsigned long long gcols = (unsigned long long)(((1u << w) - 1u) << ox) * 0x0101010101010101ull;
        const unsigned long long grows = ((h >= 8 ? ~0ull : ((1ull << (8 * h)) - 1ull)) << (8 * oy));
        if ((cols & rows & gcols & grows & alive) == 0ull) return false;
    }
    if (x0 <= 0.f && x1 >= 0.f && y0 <= 0.f && y1 >= 0.f) return true;
    if (!(n.x > 0.f) || !(n.z > 0.f)) return true;
    const float rby = -n.y * __builtin_amdgcn_rcpf(n.z), rbx = -n.y * __builtin_amdgcn_rcpf(n.x);
    auto edge_x = [&](float xe) { const float t = fminf(y1, fmaxf(y0, rby * xe)); return n.x * xe * xe + 2.f * n.y * xe * t + n.z * t * t; };
    auto edge_y = [&](float ye) { const float t = fminf(x1, fmaxf(x0, rbx * ye)); return n.x * t * t + 2.f * n.y * t * ye + n.z * ye * ye; };
    return fminf(fminf(edge_x(x0), edge_x(x1)), fminf(edge_y(y0), edge_y(y1))) <= 1.02f;
}
__global__ void __launch_bounds__(256) blend_group_stats_kernel(BlendArgs a, int ntiles, const uint32_t* __restrict__ n_contrib,
                                                                unsigned long long* __restrict__ stats) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x;
    if (tile >= ntiles) return;
    const uint2 range = a.ranges[tile];
    if (range.y <= range.x) return;
    Quadrant q;
    MGS_QUADRANT_FILL(q, a, tile, wave, lane);
    const float qx0 = q.qx0(), qy0 = q.qy0();
    // (the index formed under the condition, not q.pix: with q.pix this kernel's registers come out numbered differently)
    const uint32_t last = q.inside ? n_contrib[(size_t)q.pyi * a.W + q.pxi] : 0u;
    const uint32_t maxc = wave_max_u32(last);
    if (maxc == 0) return;
    const uint32_t end = range.x + maxc;
    // decomposition d: NG[d] groups of GW[d] x GH[d] pixels, GX[d] groups per row of groups
    constexpr int ND = 5;
    constexpr int NG[ND] = {2, 2, 4, 4, 8}, GW[ND] = {8, 4, 4, 8, 4}, GH[ND] = {4, 8, 4, 2, 2}, GX[ND] = {1, 2, 2, 1, 2};
    unsigned long long trips_step[ND] = {0, 0, 0, 0, 0}, rows[ND] = {0, 0, 0, 0, 0};
    uint32_t walk[ND][8];
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int g = 0; g < 8; ++g) walk[d][g] = 0;
    for (int b = (int)((maxc - 1) / WAVE); b >= 0; --b) {
        const uint32_t i = range.x + (uint32_t)b * WAVE + lane;
        float4 box = make_float4(0.f, 0.f, -1.f, -1.f), el = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < end) {
            const uint32_t gid_l = a.point_list[i];
            box = a.rec[(size_t)gid_l * 4];
            el = a.rec[(size_t)gid_l * 4 + 3];
        }
        const unsigned long long alive = __builtin_amdgcn_ballot_w64(last >= (uint32_t)b * WAVE + 1u);
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            int mx = 0, sum = 0;
#pragma unroll
            for (int g = 0; g < NG[d]; ++g) {
                const int ox = (g % GX[d]) * GW[d], oy = (g / GX[d]) * GH[d];
                const int n = __popcll(__builtin_amdgcn_ballot_w64(rect_hit(box, el, qx0, qy0, ox, oy, GW[d], GH[d], alive)));
                mx = max(mx, n);
                sum += n;
                walk[d][g] += (uint32_t)n;
            }
            trips_step[d] += mx;
            rows[d] += sum;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            uint32_t mx = 0;
#pragma unroll
            for (int g = 0; g < NG[d]; ++g) mx = max(mx, walk[d][g]);
            atomicAdd(stats + 8 + 3 * d + 0, trips_step[d]);
            atomicAdd(stats + 8 + 3 * d + 1, rows[d]);
            atomicAdd(stats + 8 + 3 * d + 2, (unsigned long long)mx);
        }
    }
}

int launch_blend_backward_stats(const mgs_camera& cam, const GeometryState& g, const BinningState& b,
                                const ImageState& img, unsigned long long* stats, hipStream_t s) {
    const BlendArgs a = make_args(cam, g, b, img);
    const int ntiles = a.gx * tiles_y(a.H);
    if (ntiles == 0) return 0;
    hipLaunchKernelGGL(blend_backward_stats_kernel, dim3(ntiles), dim3(256), 0, s, a, ntiles, img.n_contrib, stats);
    hipLaunchKernelGGL(blend_group_stats_kernel, dim3(ntiles), dim3(256), 0, s, a, ntiles, img.n_contrib, stats);
    MGS_HIP(hipGetLastError());
    return 0;
}

// ---- diagnostic: the forward's survivor masks against the backward's own cull (not on the hot path; mgs_debug_blend_mask_stats)
// blend_backward_s_kernel walks the masks the forward left (BinningState::fwd_masks) instead of culling for itself.  This walks
// every quadrant's list as the unsplit backward does and runs the cull the backward used to run -- the one blend_backward_stats_kernel
// and the two older backward kernels still run -- beside the forward's word of the step, trimmed to the walk's range as bs_walk
// trims it: stats[0] steps, [1] instances the own cull keeps, [2] set bits of the forward's masks, [3] instances the own cull
// keeps and the mask lacks (0: the masks cover the cull).  [2] - [1] is what the backward now evaluates for nothing.
__global__ void __launch_bounds__(256) blend_mask_stats_kernel(BlendArgs a, int ntiles, const uint32_t* __restrict__ n_contrib,
                                                               unsigned long long* __restrict__ stats) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x;
    if (tile >= ntiles) return;
    const uint2 range = a.ranges[tile];
    if (range.y <= range.x) return;
    Quadrant q;
    MGS_QUADRANT_FILL(q, a, tile, wave, lane);
    const float qx0 = q.qx0(), qy0 = q.qy0();
    const uint32_t last = q.inside ? n_contrib[q.pix] : 0u;
    const uint32_t maxc = wave_max_u32(last);
    if (maxc == 0) return;
    const uint32_t end = range.x + maxc;
    const unsigned long long* const mask_row = a.fwd_masks + fwd_mask_word(range.x, tile, wave);
    unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    const int b_first = (int)((maxc - 1) / WAVE);
    for (int b = b_first; b >= 0; --b) {
        const uint32_t i = range.x + (uint32_t)b * WAVE + lane;
        float4 box = make_float4(0.f, 0.f, -1.f, -1.f), el = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < end) {
            const uint32_t gid_l = a.point_list[i];
            box = a.rec[(size_t)gid_l * 4];
            el = a.rec[(size_t)gid_l * 4 + 3];
        }
        const unsigned long long alive = __builtin_amdgcn_ballot_w64(last >= (uint32_t)b * WAVE + 1u);
        const unsigned long long own = __builtin_amdgcn_ballot_w64(quadrant_hit(box, el, qx0, qy0, alive));
        unsigned long long fwd = mask_row[(size_t)b * 4];
        if (b == b_first) fwd &= ~0ull >> (63u - ((maxc - 1u) & 63u));
        c0 += 1;
        c1 += __popcll(own);
        c2 += __popcll(fwd);
        c3 += __popcll(own & ~fwd);
    }
    if (lane < 4) atomicAdd(stats + lane, lane == 0 ? c0 : lane == 1 ? c1 : lane == 2 ? c2 : c3);
}
int launch_blend_mask_stats(const mgs_camera& cam, const GeometryState& g, const BinningState& b,
                            const ImageState& img, unsigned long long* stats, hipStream_t s) {
    const BlendArgs a = make_args(cam, g, b, img);
    const int ntiles = a.gx * tiles_y(a.H);
    if (ntiles == 0) return 0;
    hipLaunchKernelGGL(blend_mask_stats_kernel, dim3(ntiles), dim3(256), 0, s, a, ntiles, img.n_contrib, stats);
    MGS_HIP(hipGetLastError());
    return 0;
}

// ---- diagnostic: the plain-FMA issue ceiling of this chip, measured by whoever asks (bench.py prints it next to the spec
// VALU peak).  8 waves per SIMD, every CU busy, 8 independent v_fma_f32 per trip: tools/ubench/valu_rate.hip's first row.
__global__ void __launch_bounds__(256) valu_ceiling_kernel(float* out, int iters, float seed) {
    float a0 = seed + threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
    const float c = 1.0001f, d = 0.0001f;
    for (int i = 0; i < iters; ++i) {
        a0 = __builtin_fmaf(a0, c, d); a1 = __builtin_fmaf(a1, c, d); a2 = __builtin_fmaf(a2, c, d); a3 = __builtin_fmaf(a3, c, d);
        a4 = __builtin_fmaf(a4, c, d); a5 = __builtin_fmaf(a5, c, d); a6 = __builtin_fmaf(a6, c, d); a7 = __builtin_fmaf(a7, c, d);
    }
    out[blockIdx.x * 256 + threadIdx.x] = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
}
int launch_valu_ceiling(float* out, int iters, hipStream_t s) {
    hipLaunchKernelGGL(valu_ceiling_kernel, dim3(MGS_VALU_CEILING_BLOCKS), dim3(256), 0, s, out, iters, 1.0f);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // namespace mgs
