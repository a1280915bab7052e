// What every kernel that walks a tile's instance list agrees on, stated once (blend.hip, blend_stats.hip, features.hip,
// viewer.hip).
//
// A 16x16 tile is one 256-thread workgroup whose four waves never synchronise: wave w owns the 8x8 pixel quadrant
// (w & 1, w >> 1), one pixel per lane, and walks the tile's list on its own, 64 instances per step.  The feature and viewer
// kernels trust what the blend forward left (n_contrib, the survivor masks) only because every walker forms `power` and `alpha`
// with the SAME expressions and takes a pixel by the SAME rule: they are the functions below.  (blend_backward_s_kernel writes
// the rule as instructions, bs_walk's evaluate(): keep the two in step.)
#pragma once

#include "common.h"

namespace mgs {

// ---- the falloff and the activity rule -----------------------------------------------------------------------------------
constexpr float ALPHA_MIN = 1.0f / 255.0f;      // a fragment fainter than this is skipped
constexpr float ALPHA_MAX = 0.99f;              // cap of a fragment's alpha
constexpr float T_MIN = 0.0001f;                // the forward stops a pixel BEFORE the fragment that would take T below this

// log2 of the Gaussian falloff at (dx, dy) = centre - pixel; (ca, cb, cc) as the blend record holds the conic (common.h)
__device__ __forceinline__ float falloff_power(float dx, float dy, float ca, float cb, float cc) {
    return dx * (ca * dx + cb * dy) + (cc * dy) * dy;
}
// G = exp2(power)
__device__ __forceinline__ float falloff_alpha(float op, float G) { return fminf(ALPHA_MAX, op * G); }
// Does a pixel take the fragment?  `in_walk`: the walker's own condition (the pixel's last contributor is not in front of the
// fragment), tested first.  (Written so that a NaN power or alpha counts as taken, as upstream's tests do.)
__device__ __forceinline__ bool falloff_active(bool in_walk, float power, float alpha) {
    return in_walk && !(power > 0.f) && !(alpha < ALPHA_MIN);
}

// ---- the quadrant of a wave ------------------------------------------------------------------------------------------------
struct Quadrant {
    int qx0i, qy0i;         // first pixel of the quadrant (wave-uniform when `wave` is)
    int pxi, pyi;           // the lane's pixel
    bool inside;            // ... is in the image: a pixel outside never blends
    size_t pix;             // its index in an [H][W] image
    float pxf, pyf;
    __device__ __forceinline__ float qx0() const { return (float)qx0i; }
    __device__ __forceinline__ float qy0() const { return (float)qy0i; }
};
// Fills `q`, a Quadrant declared by the caller; `a` is the kernel's argument struct (gx = tiles per row, W, H).  A macro, not a
// function: a helper is simplified on its own before it is inlined, and the kernels then come out with other operand orders and
// schedules than with these lines written in place (tools/kernel_identity.py).  x before y, fields read where they are needed:
// the order of these statements is the order the compiler schedules the kernels' set-up in.
#define MGS_QUADRANT_FILL(q, a, tile, wave, lane)                                                             \
    do {                                                                                                      \
        const int tx_ = (tile) % (a).gx, ty_ = (tile) / (a).gx;                                               \
        (q).qx0i = tx_ * TILE + ((wave) & 1) * SUB, (q).pxi = (q).qx0i + ((lane) & 7);                        \
        (q).qy0i = ty_ * TILE + ((wave) >> 1) * SUB, (q).pyi = (q).qy0i + ((lane) >> 3);                      \
        (q).inside = (q).pxi < (a).W && (q).pyi < (a).H;                                                      \
        (q).pix = (size_t)(q).pyi * (a).W + (q).pxi;                                                          \
        (q).pxf = (float)(q).pxi, (q).pyf = (float)(q).pyi;                                                   \
    } while (0)

// ---- the forward's survivor masks -----------------------------------------------------------------------------------------
// Row of the mask table that step b of `tile` takes, its list starting at range_x: range_x / 64 + tile + b.  No two tiles share
// a row: a list [x, x + n), x = 64 a + r, n = 64 c + s, takes c + (s > 0) rows from a + tile, and the next tile that has a list
// starts at a row >= a + c + (r + s) / 64 + tile + 1 (empty tiles in between only add to `tile`).
__device__ __forceinline__ size_t fwd_mask_word(uint32_t range_x, int tile, int wave) {
    return ((size_t)(range_x / WAVE) + (size_t)tile) * 4 + (size_t)wave;
}

// ---- the cull ----------------------------------------------------------------------------------------------------------------
// Does the alpha >= 1/255 ellipse of an instance reach the 8x8 pixel quadrant whose first pixel is (qx0, qy0)?
// First the padded bounding box (rejects most), then the exact minimum of the ellipse's quadratic form over the
// quadrant rectangle: the centre is inside, or the minimum lies on one of the four edges, where the quadratic is
// one-dimensional and its clamped minimiser is closed-form.  Conservative: threshold 1.02 instead of 1 and the
// rectangle grown by 0.05 px, so a skipped instance has alpha < 1/255 at every pixel of the quadrant under any
// rounding.  Runs once per lane per 64 instances, so its ~40 instructions cost < 1 per instance.
//
// `alive` is the wave's 64-bit mask of pixels that can still use an instance of this step (forward: not yet
// saturated; backward: the pixel's last contributor is not in front of the step).  An instance whose cull box covers
// no alive pixel is skipped as well -- in a dense scene most of a tile's depth range is walked for the sake of a few
// unsaturated pixels, and most instances of those steps sit over pixels that finished long ago.  Exact: a pixel
// outside the box has alpha < 1/255, a dead pixel ignores every instance.
__device__ __forceinline__ bool quadrant_hit(const float4 c /* px, py, ex, ey */, const float4 n /* na, nb, nc, . */,
                                             float qx0, float qy0, unsigned long long alive) {
    const float x0 = qx0 - 0.05f - c.x, x1 = qx0 + (float)(SUB - 1) + 0.05f - c.x;   // rectangle relative to the centre
    const float y0 = qy0 - 0.05f - c.y, y1 = qy0 + (float)(SUB - 1) + 0.05f - c.y;
    if (c.z < 0.f) return false;                      // opacity < 1/255 (or an empty slot): contributes nowhere
    if (!((c.z >= x0) && (-c.z <= x1) && (c.w >= y0) && (-c.w <= y1))) return false;   // bounding boxes apart
    {   // pixels (qx0 + i, qy0 + j) inside the box: i in [ix0, ix1], j in [iy0, iy1] (clamped; the box may be huge or NaN-wide)
        const int ix0 = (int)fminf(8.f, fmaxf(0.f, ceilf(-x0 - c.z - 0.06f))), ix1 = (int)fminf(7.f, fmaxf(-1.f, floorf(-x0 + c.z + 0.06f)));
        const int iy0 = (int)fminf(8.f, fmaxf(0.f, ceilf(-y0 - c.w - 0.06f))), iy1 = (int)fminf(7.f, fmaxf(-1.f, floorf(-y0 + c.w + 0.06f)));
        if (ix0 > ix1 || iy0 > iy1) return false;
        const unsigned long long cols = (unsigned long long)((0xFFu >> (7 - ix1)) & (0xFFu << ix0) & 0xFFu) * 0x0101010101010101ull;
        const unsigned long long rows = (~0ull >> (8 * (7 - iy1))) & (~0ull << (8 * iy0));
        if ((cols & rows & alive) == 0ull) return false;
    }
    if (x0 <= 0.f && x1 >= 0.f && y0 <= 0.f && y1 >= 0.f) return true;                 // centre inside
    if (!(n.x > 0.f) || !(n.z > 0.f)) return true;                                     // no ellipse data: keep
    // v_rcp_f32 (1 ulp) instead of two IEEE divide sequences: the 2 % threshold margin dwarfs the error
    const float rby = -n.y * __builtin_amdgcn_rcpf(n.z), rbx = -n.y * __builtin_amdgcn_rcpf(n.x);
    auto edge_x = [&](float xe) {          // x = xe, y in [y0, y1]
        const float t = fminf(y1, fmaxf(y0, rby * xe));
        return n.x * xe * xe + 2.f * n.y * xe * t + n.z * t * t;
    };
    auto edge_y = [&](float ye) {          // y = ye, x in [x0, x1]
        const float t = fminf(x1, fmaxf(x0, rbx * ye));
        return n.x * t * t + 2.f * n.y * t * ye + n.z * ye * ye;
    };
    const float qmin = fminf(fminf(edge_x(x0), edge_x(x1)), fminf(edge_y(y0), edge_y(y1)));
    return qmin <= 1.02f;
}

// ---- a survivor's record through the scalar cache (wave-uniform address -> s_load) ------------------------------------------
struct Rec {
    float px, py, ca, cb, cc, op, r, g, b, z;
};
// Read through the CONSTANT address space (common.h): the backend then always selects scalar loads for the wave-uniform
// address (s_load_dwordx2 + s_load_dwordx8).  Through the generic pointer that choice hangs on a no-clobber analysis that
// flips to per-lane vector loads with unrelated edits of the loop (an atomic moved, an LDS store added).  The records
// are written by preprocess, an earlier kernel.
__device__ __forceinline__ Rec fetch(const float* rec, uint32_t gid_uniform) {
    const const_float_p p = MGS_CONST(rec) + (size_t)gid_uniform * REC_FLOATS;
    return Rec{p[R_X], p[R_Y], p[R_CA], p[R_CB], p[R_CC], p[R_OPAC], p[R_R], p[R_G], p[R_B], p[R_DEPTH]};
}

// ---- what the blend kernels are handed ---------------------------------------------------------------------------------------
// (BS_TRACE, a diagnostic build of blend.hip alone, adds a member: no BlendArgs value crosses a translation unit, and
//  make_args has internal linkage)
struct BlendArgs {
#ifdef BS_TRACE
    unsigned long long* trace;
#endif
    const float4* __restrict__ rec;            // [P][4]
    const uint32_t* __restrict__ point_list;
    const uint2* __restrict__ ranges;
    const float* __restrict__ bg;
    unsigned long long* fwd_masks;             // BinningState::fwd_masks: [row][quadrant], the forward's survivor masks
    int W, H, gx;
};
static inline BlendArgs make_args(const mgs_camera& cam, const GeometryState& g, const BinningState& b,
                                  const ImageState& img) {
    BlendArgs a;
#ifdef BS_TRACE
    a.trace = nullptr;
#endif
    a.rec = reinterpret_cast<const float4*>(g.rec);
    a.point_list = b.vals_sorted;
    a.ranges = img.ranges;
    a.bg = cam.bg;
    a.fwd_masks = b.fwd_masks;
    a.W = cam.image_width;
    a.H = cam.image_height;
    a.gx = tiles_x(a.W);
    return a;
}

}  // namespace mgs
