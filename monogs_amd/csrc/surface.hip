// Surface depth: the median depth and the depth variance of every pixel through the tables of a finished forward, and the
// normals of a depth image ("Surface depth").
//
// Boundary replaced: the reference renders one depth, the alpha-blended mean sum w z, and never
// builds a surface from its map.  A blended mean mixes the layers a ray crosses; what mesh fusion wants is the depth of the
// contributor at which the transmittance falls through one half, and a measure of how wide the ray's depth distribution is.
// Neither is linear in per-Gaussian values, so mgs_features_forward cannot produce them: they take a walk of their own.
//
// What is read, and never written: what features.hip reads (feat_walk.h: the blend records, the point list in blend order, the
// canonical ranges, n_contrib, final_T, the forward's survivor masks), so the kernel is valid after an exact or a
// capacity-mode forward, on either binning path, before or after the backward.
//
// gfx950 mapping: that of features_forward_kernel.  One 256-thread workgroup per tile, four waves that never synchronise, one
// wave per 8x8 quadrant, one pixel per lane; the step's survivor word and the survivor's record (centre, conic, opacity,
// depth) arrive through scalar loads, the 64 lanes form alpha with tile_walk.h's falloff.  The loop is written here and not
// taken from feat_walk: the callback of that walk sees (gid, w) only, and this one needs the transmittance after the step and a
// way out of the loop.  No LDS, no atomics, no barriers.
#include "common.h"
#include "feat_walk.h"         // FeatArgs, feat_quadrant, make_feat_args
#include "tile_walk.h"

#include <math.h>

// Where the early leave is tested: 1 = after every survivor, 0 = once per 64-instance step only (DESIGN.md section 3 has both timed)
#ifndef MGS_SURFACE_LEAVE_PER_SURVIVOR
#define MGS_SURFACE_LEAVE_PER_SURVIVOR 1
#endif

namespace mgs {

namespace {

// VAR: the three sums of the variance are carried and depth_var is written.  LEAVE: a wave leaves once every pixel of its
// quadrant has its median or has passed its last contributor (median only, no variance gate).  MED: the median planes are written.
template <bool MED, bool VAR, bool LEAVE>
__global__ void __launch_bounds__(256) surface_depth_kernel(FeatArgs a, float min_opacity, float max_var,
                                                            float* __restrict__ median_depth, int32_t* __restrict__ median_id,
                                                            float* __restrict__ depth_var) {
    static_assert(!LEAVE || (MED && !VAR), "the early leave is for the median alone");
    const FeatQuad q = feat_quadrant(a);
    float T = 1.f, z_m = 0.f, z_1 = 0.f, S1 = 0.f, S2 = 0.f, O = 0.f;
    int id_m = -1;
    bool found = false, first = true;
    bool leave = false;             // wave-uniform
    if (q.maxc != 0u) {
        const const_float_p recs = MGS_CONST(a.rec);
        const const_u64_p mask_row = MGS_CONST_U64(a.fwd_masks) + fwd_mask_word(q.range.x, q.tile, q.wave);
        const uint32_t end = q.range.x + q.maxc;
        const int b_last = (int)((q.maxc - 1u) / WAVE);
        for (int b = 0; b <= b_last; ++b) {
            unsigned long long mask = mask_row[(size_t)b * 4];
            if (b == b_last) mask &= ~0ull >> (63u - ((q.maxc - 1u) & 63u));   // positions behind the quadrant's last contributor
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
                const float z = r[R_DEPTH];                     // wave-uniform: the record's float, as it is
                if (VAR) {
                    if (act && first) z_1 = z, first = false;
                    const float w = a_eff * T, d = z - z_1;
                    O += w;
                    S1 += w * d;
                    S2 += (w * d) * d;
                }
                T = T * (1.f - a_eff);                          // t_i, formed as every walker forms its T
                if (MED && act && !found && T <= 0.5f) found = true, z_m = z, id_m = (int)gid;
                // (per survivor: ... or its last contributor is this instance or one in front of it)
                if (LEAVE && MGS_SURFACE_LEAVE_PER_SURVIVOR && __builtin_amdgcn_ballot_w64(!found && j < rel_last) == 0ull) {
                    leave = true;
                    break;
                }
            }
            // nothing left to learn: every pixel has its median, or its last contributor lies in a step already walked
            if (LEAVE && (leave || __builtin_amdgcn_ballot_w64(!found && rel_last >= WAVE) == 0ull)) break;
        }
    }
    if (!q.inside) return;
    float var = 0.f;
    if (VAR) {
        if (O > 0.f) {
            const float m = S1 / O;
            var = fmaxf(0.f, S2 / O - m * m);
        }
        depth_var[q.pix] = var;
    }
    if (MED) {
        const bool cleared = (1.0f - a.final_T[q.pix] < min_opacity) || (VAR && max_var > 0.f && var > max_var);
        median_depth[q.pix] = cleared ? 0.f : z_m;
        if (median_id) median_id[q.pix] = cleared ? -1 : id_m;
    }
}

// no Gaussians: no median, no spread
__global__ void __launch_bounds__(256) surface_empty_kernel(float* __restrict__ median_depth, int32_t* __restrict__ median_id,
                                                            float* __restrict__ depth_var, size_t HW) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += stride) {
        if (median_depth) median_depth[i] = 0.f;
        if (median_id) median_id[i] = -1;
        if (depth_var) depth_var[i] = 0.f;
    }
}

// ---- normals of a depth image -------------------------------------------------------------------------------------------------
// One lane per pixel; the five depths through plain loads (a row is contiguous across a wave), three coalesced plane stores; the
// border and the gates are zeros written by the same lane.  Every operation is a single IEEE float32 one, in the order the
// specification writes them (no contraction): a float32 restatement on the host gives the same bits.
struct Vec3 {
    float x, y, z;
};
#pragma clang fp contract(off)
__device__ __forceinline__ Vec3 pixel_point(float d, int x, int y, float fx, float fy, float cx, float cy) {
    return Vec3{d * (((float)x + 0.5f - cx) / fx), d * (((float)y + 0.5f - cy) / fy), d};
}

__global__ void __launch_bounds__(256) depth_normals_kernel(int W, int H, const float* __restrict__ depth, float fx, float fy,
                                                            float cx, float cy, float max_jump, float* __restrict__ normals) {
    const size_t HW = (size_t)W * H, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const int x = (int)(i % (size_t)W), y = (int)(i / (size_t)W);
    Vec3 n{0.f, 0.f, 0.f};
    if (x > 0 && y > 0 && x < W - 1 && y < H - 1) {
        const float dc = depth[i], dl = depth[i - 1], dr = depth[i + 1], du = depth[i - (size_t)W], dd = depth[i + (size_t)W];
        bool ok = dc > 0.f && dl > 0.f && dr > 0.f && du > 0.f && dd > 0.f;        // (a NaN depth is invalid)
        if (max_jump > 0.f)
            ok = ok && !(fabsf(dl - dc) > max_jump) && !(fabsf(dr - dc) > max_jump) && !(fabsf(du - dc) > max_jump) &&
                 !(fabsf(dd - dc) > max_jump);
        if (ok) {
            const Vec3 pc = pixel_point(dc, x, y, fx, fy, cx, cy);
            const Vec3 pl = pixel_point(dl, x - 1, y, fx, fy, cx, cy), pr = pixel_point(dr, x + 1, y, fx, fy, cx, cy);
            const Vec3 pu = pixel_point(du, x, y - 1, fx, fy, cx, cy), pd = pixel_point(dd, x, y + 1, fx, fy, cx, cy);
            const Vec3 u{pr.x - pl.x, pr.y - pl.y, pr.z - pl.z}, v{pd.x - pu.x, pd.y - pu.y, pd.z - pu.z};
            const Vec3 c{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
            const float len = sqrtf(c.x * c.x + c.y * c.y + c.z * c.z);
            if (len > 0.f && len < INFINITY) {
                n = Vec3{c.x / len, c.y / len, c.z / len};
                if (n.x * pc.x + n.y * pc.y + n.z * pc.z > 0.f) n = Vec3{-n.x, -n.y, -n.z};
            }
        }
    }
    normals[i] = n.x;
    normals[HW + i] = n.y;
    normals[2 * HW + i] = n.z;
}

}  // namespace

}  // namespace mgs

extern "C" int mgs_surface_depth(const mgs_camera* cam, int32_t P, uint64_t num_rendered, const void* geometry,
                                 const void* binning, const void* image, int32_t want, float min_opacity, float max_std,
                                 float* median_depth, int32_t* median_id, float* depth_var, void* stream) {
    using namespace mgs;
    const char* who = "mgs_surface_depth";
    if (check_cam(cam, who)) return 1;
    if (P < 0) { set_error("%s: P must be >= 0", who); return 1; }
    if (check_map_size(P, who)) return 1;
    if (want == 0 || (want & ~(MGS_SURFACE_MEDIAN | MGS_SURFACE_VARIANCE))) {
        set_error("%s: want must be a non-empty sum of MGS_SURFACE_MEDIAN and MGS_SURFACE_VARIANCE (got %d)", who, want);
        return 1;
    }
    const bool med = want & MGS_SURFACE_MEDIAN, var = want & MGS_SURFACE_VARIANCE;
    if (med && !median_depth) { set_error("%s: MGS_SURFACE_MEDIAN needs median_depth", who); return 1; }
    if (var && !depth_var) { set_error("%s: MGS_SURFACE_VARIANCE needs depth_var", who); return 1; }
    if (!(min_opacity >= 0.f)) { set_error("%s: min_opacity must be >= 0 and not NaN", who); return 1; }
    if (!(max_std >= 0.f)) { set_error("%s: max_std must be >= 0 and not NaN", who); return 1; }
    if (max_std > 0.f && !var) { set_error("%s: max_std > 0 needs MGS_SURFACE_VARIANCE and depth_var", who); return 1; }
    const int W = cam->image_width, H = cam->image_height;
    const int ntiles = tiles_x(W) * tiles_y(H);
    hipStream_t s = (hipStream_t)stream;
    if (!med) median_depth = nullptr, median_id = nullptr;
    if (!var) depth_var = nullptr;
    if (P == 0) {
        const size_t HW = (size_t)W * H;
        const size_t blocks = (HW + 255) / 256 > 4096 ? 4096 : (HW + 255) / 256;
        hipLaunchKernelGGL(surface_empty_kernel, dim3((unsigned)blocks), dim3(256), 0, s, median_depth, median_id, depth_var, HW);
        MGS_HIP(hipGetLastError());
        return 0;
    }
    if (!geometry || !image) { set_error("%s: geometry, image must be non-NULL", who); return 1; }
    if (num_rendered > 0 && !binning) { set_error("%s: binning scratch is NULL", who); return 1; }
    const auto [g, img, b] = carve_forward(geometry, binning, image, P, num_rendered, W, H);
    const FeatArgs a = make_feat_args(*cam, 0, g, b, img);
    const float max_var = max_std * max_std;
#define SURFACE(MED_, VAR_, LEAVE_)                                                                                        \
    hipLaunchKernelGGL((surface_depth_kernel<MED_, VAR_, LEAVE_>), dim3(ntiles), dim3(256), 0, s, a, min_opacity, max_var, \
                       median_depth, median_id, depth_var)
    if (med && var) SURFACE(true, true, false);
    else if (med) SURFACE(true, false, true);
    else SURFACE(false, true, false);
#undef SURFACE
    MGS_HIP(hipGetLastError());
    return 0;
}

extern "C" int mgs_depth_normals(int32_t W, int32_t H, const float* depth, float fx, float fy, float cx, float cy, float max_jump,
                                 float* normals, void* stream) {
    using namespace mgs;
    const char* who = "mgs_depth_normals";
    if (W <= 0 || H <= 0 || (uint64_t)W * (uint64_t)H >= (1ull << 31)) {
        set_error("%s: W, H must be positive and W x H < 2^31 (got %d x %d)", who, W, H);
        return 1;
    }
    if (!depth || !normals) { set_error("%s: depth, normals must be non-NULL", who); return 1; }
    if (!(fx > 0.f) || !(fy > 0.f) || !(fx < INFINITY) || !(fy < INFINITY) || cx != cx || cy != cy) {
        set_error("%s: fx, fy must be positive and finite, cx, cy not NaN", who);
        return 1;
    }
    if (!(max_jump >= 0.f)) { set_error("%s: max_jump must be >= 0 and not NaN", who); return 1; }
    const size_t HW = (size_t)W * H;
    hipLaunchKernelGGL(depth_normals_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, H, depth, fx,
                       fy, cx, cy, max_jump, normals);
    MGS_HIP(hipGetLastError());
    return 0;
}
