// The walk of a finished forward's tile lists that the feature kernels (features.hip) and the pose-tangent blend (pose_tangent.hip)
// share: the arguments, what a wave knows about its quadrant, and the loop over the survivors the blend forward left.  In the unnamed
// namespace: each unit that includes this compiles its own copy, under its own flags.
#pragma once

#include "common.h"
#include "tile_walk.h"

namespace mgs {

namespace {

struct FeatArgs {
    const float* __restrict__ rec;                  // [P][16]
    const uint32_t* __restrict__ point_list;
    const uint2* __restrict__ ranges;               // canonical: {0, 0} for an empty tile
    const unsigned long long* __restrict__ fwd_masks;
    const float* __restrict__ final_T;
    const uint32_t* __restrict__ n_contrib;
    int W, H, gx, K;
};

// what a wave knows about its quadrant before it walks
struct FeatQuad : Quadrant {
    uint2 range;            // wave-uniform
    uint32_t last, maxc;    // the pixel's n_contrib; its maximum over the quadrant (wave-uniform)
    int tile, wave, lane;
};

__device__ __forceinline__ FeatQuad feat_quadrant(const FeatArgs& a) {
    FeatQuad q;
    q.tile = (int)blockIdx.x;
    q.wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    q.lane = (int)(threadIdx.x & 63);
    MGS_QUADRANT_FILL(q, a, q.tile, q.wave, q.lane);   // (a pixel outside the image never blends: last = 0)
    const uint2 r = a.ranges[q.tile];
    q.range = make_uint2((uint32_t)__builtin_amdgcn_readfirstlane((int)r.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)r.y));
    q.last = q.inside && q.range.y > q.range.x ? a.n_contrib[q.pix] : 0u;
    q.maxc = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(q.last));
    return q;
}

// The walk both kernels share: use(gid, w) is called, by all 64 lanes, for every survivor at least one pixel of the quadrant
// takes; gid is wave-uniform, w = alpha T of the lane's pixel (0 where the pixel does not take the instance).  Only steps the
// forward entered are read: a pixel whose last contributor sits in step b was live when the forward began step b.
template <class F>
__device__ __forceinline__ void feat_walk(const FeatArgs& a, const FeatQuad& q, F&& use) {
    const const_float_p recs = MGS_CONST(a.rec);
    const const_u64_p mask_row = MGS_CONST_U64(a.fwd_masks) + fwd_mask_word(q.range.x, q.tile, q.wave);
    const uint32_t end = q.range.x + q.maxc;
    const int b_last = (int)((q.maxc - 1u) / WAVE);
    float T = 1.f;
    for (int b = 0; b <= b_last; ++b) {
        unsigned long long mask = mask_row[(size_t)b * 4];
        if (b == b_last) mask &= ~0ull >> (63u - ((q.maxc - 1u) & 63u));       // positions behind the quadrant's last contributor
        const uint32_t i = q.range.x + (uint32_t)b * WAVE + (uint32_t)q.lane;
        const uint32_t gid_l = i < end ? a.point_list[i] : 0u;
        // instance j of the step has the 1-based list position b * 64 + j + 1: "position <= last" as one compare with j
        const int rel_last = (int)q.last - (int)((uint32_t)b * WAVE + 1u);
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            const uint32_t gid = bcast(gid_l, j);
            const const_float_p r = recs + (size_t)gid * REC_FLOATS;
            const float dx = r[R_X] - q.pxf, dy = r[R_Y] - q.pyf;
            const float power = falloff_power(dx, dy, r[R_CA], r[R_CB], r[R_CC]);
            const float alpha = falloff_alpha(r[R_OPAC], __builtin_amdgcn_exp2f(power));
            const bool act = falloff_active(j <= rel_last, power, alpha);
            if (__builtin_amdgcn_ballot_w64(act) == 0ull) continue;
            const float a_eff = act ? alpha : 0.f;          // a pixel that passes: w = 0, T * (1 - 0) = T
            const float w = a_eff * T;
            T = T * (1.f - a_eff);
            use(gid, w);
        }
    }
}

inline FeatArgs make_feat_args(const mgs_camera& cam, int K, const GeometryState& g, const BinningState& b,
                               const ImageState& img) {
    FeatArgs a;
    a.rec = g.rec;
    a.point_list = b.vals_sorted;
    a.ranges = img.ranges;
    a.fwd_masks = b.fwd_masks;
    a.final_T = img.final_T;
    a.n_contrib = img.n_contrib;
    a.W = cam.image_width;
    a.H = cam.image_height;
    a.gx = tiles_x(a.W);
    a.K = K;
    return a;
}

}  // namespace

}  // namespace mgs
