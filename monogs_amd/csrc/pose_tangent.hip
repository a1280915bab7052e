// Pose-tangent rendering: the per-pixel Jacobian of (R, G, B, depth, opacity) with respect to the six pose tangents
// tau = (rho, theta) of T_cw(tau) = exp(tau^) T_cw at tau = 0 -- a FORWARD-mode pass through the rasteriser, walked through the
// lists and survivor masks of a finished forward ("Pose tangents").  The tangent blend is a feat_walk
// (feat_walk.h) with 30 accumulators per lane; it forms alpha with tile_walk.h's falloff and is compiled with features.hip's flags.
//
// Boundary replaced: the reference tracks with first-order Adam steps on the summed gradient (utils/slam_tracker.py:142-176
// there); it has no per-pixel Jacobian.  The conventions are the backward's: decisions, radii and rectangles are constants, a
// view-space ratio clamped at 1.3 tanfov is a constant, the 0.99 cap of alpha is straight-through.
//
// Two launches:
//   pose_tangent_records_kernel   one lane per Gaussian with radii > 0: d(px, py, ka, kb, kc, z) / d tau_k, k = 0..5, as three
//                                 64-byte lines [k][8] (floats 6, 7 of a direction unused).  (ka, kb, kc) are the blend
//                                 record's log2-scaled conic (common.h), so the walk forms d power in the units of `power`.
//   pose_tangent_blend_kernel     one 256-thread workgroup per tile, four independent waves, one pixel per lane; blend and tangent
//                                 record of a survivor through the scalar cache; no LDS, no barriers, no atomics.
#include "common.h"
#include "feat_walk.h"
#include "tile_walk.h"

namespace mgs {

constexpr int TAN_FLOATS = 48;          // per-Gaussian tangent record: three 64-byte lines, direction k at floats [8 k, 8 k + 6)
constexpr int TAN_DIR = 8;
enum : int { TN_PX = 0, TN_PY = 1, TN_KA = 2, TN_KB = 3, TN_KC = 4, TN_Z = 5 };

namespace {

struct TanRecArgs {
    const float *means3D, *scales, *rotations, *cov3D;
    const int32_t* radii;
    const float *V, *PM, *PR;
    float* tan;               // [P][TAN_FLOATS]
    float tanfovx, tanfovy, focal_x, focal_y, mod;
    int P, W, H, iso;
};

// Sigma = R S^2 R^T, the six upper-triangular entries (preprocess.hip's cov3d_from_scale_rot; only its value is needed here)
__device__ __forceinline__ void tan_cov3d(const float s[3], const float q[4], float mod, float cov[6]) {
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    const float Rm[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                         2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                         2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)};
    float Mm[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        Mm[3 * i + 0] = Rm[3 * i + 0] * (s[0] * mod);
        Mm[3 * i + 1] = Rm[3 * i + 1] * (s[1] * mod);
        Mm[3 * i + 2] = Rm[3 * i + 2] * (s[2] * mod);
    }
    auto e = [&](int i, int j) { return (Mm[3 * i] * Mm[3 * j] + Mm[3 * i + 1] * Mm[3 * j + 1]) + Mm[3 * i + 2] * Mm[3 * j + 2]; };
    cov[0] = e(0, 0); cov[1] = e(0, 1); cov[2] = e(0, 2);
    cov[3] = e(1, 1); cov[4] = e(1, 2); cov[5] = e(2, 2);
}

__device__ __forceinline__ void cross3(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// With t = W m + T:  dt/drho_k = e_k, dt/dtheta_k = e_k x t;  dW/dtheta_k = [e_k]x W, dW/drho_k = 0.  The 2x3 matrix of the EWA
// projection is Tm = Jm W, so dTm = (dJm + Jm [e_k]x) W: row a of Jm [e_k]x is Jm_a x e_k.  cov = Tm Sigma Tm^T + 0.3 I gives
// dcov_ab = dTm_a . U_b + dTm_b . U_a with U_a = Sigma Tm_a, and d conic = -conic dcov conic.
__global__ void __launch_bounds__(256) pose_tangent_records_kernel(TanRecArgs a) {
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    if (idx >= a.P) return;
    if (a.radii[idx] <= 0) return;            // never read by the walk: its lines stay as they are
    const const_float_p V = MGS_CONST(a.V), PM = MGS_CONST(a.PM), PR = MGS_CONST(a.PR);
    const float x = a.means3D[3 * (size_t)idx], y = a.means3D[3 * (size_t)idx + 1], z = a.means3D[3 * (size_t)idx + 2];
    float t[3], ph[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = ((V[k] * x + V[4 + k] * y) + V[8 + k] * z) + V[12 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) ph[k] = ((PM[k] * x + PM[4 + k] * y) + PM[8 + k] * z) + PM[12 + k];
    const float p_w = 1.0f / (ph[3] + 0.0000001f);
    const float projx = ph[0] * p_w, projy = ph[1] * p_w;

    float cov[6];
    if (a.cov3D) {
#pragma unroll
        for (int k = 0; k < 6; ++k) cov[k] = a.cov3D[6 * (size_t)idx + k];
    } else {
        const float* sp = a.scales + (a.iso ? (size_t)idx : 3 * (size_t)idx);
        const float s[3] = {sp[0], sp[a.iso ? 0 : 1], sp[a.iso ? 0 : 2]};
        const float* qp = a.rotations + 4 * (size_t)idx;
        const float q[4] = {qp[0], qp[1], qp[2], qp[3]};
        tan_cov3d(s, q, a.mod, cov);
    }
    // ---- the forward's projection (preprocess.hip, project_cov)
    const float limx = 1.3f * a.tanfovx, limy = 1.3f * a.tanfovy;
    const float tz = t[2], itz = 1.0f / tz;
    const float txtz = t[0] * itz, tytz = t[1] * itz;
    const bool clamp_x = (txtz < -limx) || (txtz > limx), clamp_y = (tytz < -limy) || (tytz > limy);
    const float tx = fminf(limx, fmaxf(-limx, txtz)) * tz, ty = fminf(limy, fmaxf(-limy, tytz)) * tz;
    const float itz2 = itz * itz;
    const float J0[3] = {a.focal_x * itz, 0.f, -(a.focal_x * tx) * itz2};
    const float J1[3] = {0.f, a.focal_y * itz, -(a.focal_y * ty) * itz2};
    auto Wm = [&](int i, int j) { return V[4 * j + i]; };          // rotation block of T_cw
    float T0[3], T1[3], U0[3], U1[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        T0[j] = J0[0] * Wm(0, j) + J0[2] * Wm(2, j);
        T1[j] = J1[1] * Wm(1, j) + J1[2] * Wm(2, j);
    }
    const float S[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        U0[j] = (T0[0] * S[0][j] + T0[1] * S[1][j]) + T0[2] * S[2][j];
        U1[j] = (T1[0] * S[0][j] + T1[1] * S[1][j]) + T1[2] * S[2][j];
    }
    const float cxx = ((U0[0] * T0[0] + U0[1] * T0[1]) + U0[2] * T0[2]) + 0.3f;
    const float cxy = (U0[0] * T1[0] + U0[1] * T1[1]) + U0[2] * T1[2];
    const float cyy = ((U1[0] * T1[0] + U1[1] * T1[1]) + U1[2] * T1[2]) + 0.3f;
    const float det_inv = 1.f / (cxx * cyy - cxy * cxy);
    const float ca = cyy * det_inv, cb = -cxy * det_inv, cc = cxx * det_inv;

    constexpr float LOG2E = 1.4426950408889634f;
    float4* out = reinterpret_cast<float4*>(a.tan + (size_t)idx * TAN_FLOATS);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float e[3] = {(k % 3) == 0 ? 1.f : 0.f, (k % 3) == 1 ? 1.f : 0.f, (k % 3) == 2 ? 1.f : 0.f};
        float dt[3], A0[3] = {0.f, 0.f, 0.f}, A1[3] = {0.f, 0.f, 0.f};
        if (k < 3) {
            dt[0] = e[0]; dt[1] = e[1]; dt[2] = e[2];
        } else {
            cross3(e, t, dt);
            cross3(J0, e, A0);
            cross3(J1, e, A1);
        }
        // pixel centre through the raw projection: ph = P (t, 1), P[r][j] = PR[4 j + r]
        const float dph0 = (PR[0] * dt[0] + PR[4] * dt[1]) + PR[8] * dt[2];
        const float dph1 = (PR[1] * dt[0] + PR[5] * dt[1]) + PR[9] * dt[2];
        const float dph3 = (PR[3] * dt[0] + PR[7] * dt[1]) + PR[11] * dt[2];
        const float dpx = 0.5f * (float)a.W * (p_w * (dph0 - projx * dph3));
        const float dpy = 0.5f * (float)a.H * (p_w * (dph1 - projy * dph3));
        const float dz = dt[2];
        const float dtx = clamp_x ? 0.f : dt[0], dty = clamp_y ? 0.f : dt[1];
        // dJm: J00 = fx / tz, J02 = -fx tx / tz^2 (tx the clamped value), likewise y
        A0[0] += -J0[0] * itz * dz;
        A0[2] += -a.focal_x * itz2 * dtx - 2.f * J0[2] * itz * dz;
        A1[1] += -J1[1] * itz * dz;
        A1[2] += -a.focal_y * itz2 * dty - 2.f * J1[2] * itz * dz;
        float dT0[3], dT1[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            dT0[j] = (A0[0] * Wm(0, j) + A0[1] * Wm(1, j)) + A0[2] * Wm(2, j);
            dT1[j] = (A1[0] * Wm(0, j) + A1[1] * Wm(1, j)) + A1[2] * Wm(2, j);
        }
        const float dxx = 2.f * ((dT0[0] * U0[0] + dT0[1] * U0[1]) + dT0[2] * U0[2]);
        const float dxy = ((dT0[0] * U1[0] + dT0[1] * U1[1]) + dT0[2] * U1[2]) + ((dT1[0] * U0[0] + dT1[1] * U0[1]) + dT1[2] * U0[2]);
        const float dyy = 2.f * ((dT1[0] * U1[0] + dT1[1] * U1[1]) + dT1[2] * U1[2]);
        // d conic = -C dcov C,  C = [[ca, cb], [cb, cc]], dcov = [[dxx, dxy], [dxy, dyy]]
        const float m00 = ca * dxx + cb * dxy, m01 = ca * dxy + cb * dyy;
        const float m10 = cb * dxx + cc * dxy, m11 = cb * dxy + cc * dyy;
        const float da = -(m00 * ca + m01 * cb), db = -(m00 * cb + m01 * cc), dc = -(m10 * cb + m11 * cc);
        out[2 * k] = make_float4(dpx, dpy, -0.5f * LOG2E * da, -LOG2E * db);
        out[2 * k + 1] = make_float4(-0.5f * LOG2E * dc, dz, 0.f, 0.f);
    }
}

// The tangent blend.  Per contributor i of a pixel, in blend order (S_k starts at 0):
//   d power_k = dka dx^2 + dkb dx dy + dkc dy^2 + (2 ka dx + kb dy) dpx + (kb dx + 2 kc dy) dpy      (log2 units, like `power`)
//   d alpha_k = ln2 opacity G d power_k                  (straight-through where alpha is capped)
//   w_k = T (d alpha_k - alpha S_k);  dC_k += c w_k;  dD_k += z w_k + dz_k alpha T;  S_k += d alpha_k / (1 - alpha)
// and at the end dT_final,k = -T_final S_k: dC_k += bg dT_final,k, dO_k = T_final S_k.  NDIR directions per walk, k0 the first.
template <int NDIR>
__device__ __forceinline__ void tangent_walk(const FeatArgs& a, const FeatQuad& q, const float* tan, const float* bg, float* J,
                                             int k0) {
    float dC[NDIR][3], dD[NDIR], S[NDIR];
#pragma unroll
    for (int k = 0; k < NDIR; ++k) dC[k][0] = dC[k][1] = dC[k][2] = dD[k] = S[k] = 0.f;
    if (q.maxc != 0u) {
        const const_float_p recs = MGS_CONST(a.rec), tans = MGS_CONST(tan);
        const const_u64_p mask_row = MGS_CONST_U64(a.fwd_masks) + fwd_mask_word(q.range.x, q.tile, q.wave);
        const uint32_t end = q.range.x + q.maxc;
        const int b_last = (int)((q.maxc - 1u) / WAVE);
        float T = 1.f;
        for (int b = 0; b <= b_last; ++b) {
            unsigned long long mask = mask_row[(size_t)b * 4];
            if (b == b_last) mask &= ~0ull >> (63u - ((q.maxc - 1u) & 63u));
            const uint32_t i = q.range.x + (uint32_t)b * WAVE + (uint32_t)q.lane;
            const uint32_t gid_l = i < end ? a.point_list[i] : 0u;
            const int rel_last = (int)q.last - (int)((uint32_t)b * WAVE + 1u);
            while (mask) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                const uint32_t gid = bcast(gid_l, j);
                const const_float_p r = recs + (size_t)gid * REC_FLOATS;
                const float dx = r[R_X] - q.pxf, dy = r[R_Y] - q.pyf;
                const float ka = r[R_CA], kb = r[R_CB], kc = r[R_CC];
                const float power = falloff_power(dx, dy, ka, kb, kc);
                const float G = __builtin_amdgcn_exp2f(power);
                const float alpha = falloff_alpha(r[R_OPAC], G);
                const bool act = falloff_active(j <= rel_last, power, alpha);
                if (__builtin_amdgcn_ballot_w64(act) == 0ull) continue;
                const float a_eff = act ? alpha : 0.f;          // a pixel that passes: every term below is 0, T and S stay
                const float h = act ? 0.6931471805599453f * (r[R_OPAC] * G) : 0.f;
                const float aT = a_eff * T;
                const float inv = __builtin_amdgcn_rcpf(1.f - a_eff);
                const float u = dx * dx, v = dx * dy, w = dy * dy;
                const float gx = 2.f * ka * dx + kb * dy, gy = kb * dx + 2.f * kc * dy;
                const float cr = r[R_R], cg = r[R_G], cbl = r[R_B], zd = r[R_DEPTH];
                const const_float_p tr = tans + (size_t)gid * TAN_FLOATS + (size_t)k0 * TAN_DIR;
#pragma unroll
                for (int k = 0; k < NDIR; ++k) {
                    const const_float_p d = tr + k * TAN_DIR;
                    const float dp = u * d[TN_KA] + v * d[TN_KB] + w * d[TN_KC] + gx * d[TN_PX] + gy * d[TN_PY];
                    const float da = h * dp;
                    const float wk = T * (da - a_eff * S[k]);
                    dC[k][0] += cr * wk;
                    dC[k][1] += cg * wk;
                    dC[k][2] += cbl * wk;
                    dD[k] += zd * wk + d[TN_Z] * aT;
                    S[k] += da * inv;
                }
                T = T * (1.f - a_eff);
            }
        }
    }
    if (!q.inside) return;
    const size_t HW = (size_t)a.H * a.W;
    const float Tf = a.final_T[q.pix];
    const const_float_p bgc = MGS_CONST(bg);
#pragma unroll
    for (int k = 0; k < NDIR; ++k) {
        float* o = J + (size_t)(5 * (k0 + k)) * HW + q.pix;
        const float dO = Tf * S[k];
        o[0] = dC[k][0] - bgc[0] * dO;
        o[HW] = dC[k][1] - bgc[1] * dO;
        o[2 * HW] = dC[k][2] - bgc[2] * dO;
        o[3 * HW] = dD[k];
        o[4 * HW] = dO;
    }
}

template <int NDIR>
__global__ void __launch_bounds__(256) pose_tangent_blend_kernel(FeatArgs a, const float* __restrict__ tan,
                                                                 const float* __restrict__ bg, float* __restrict__ J) {
    const FeatQuad q = feat_quadrant(a);
#pragma unroll 1
    for (int k0 = 0; k0 < 6; k0 += NDIR) tangent_walk<NDIR>(a, q, tan, bg, J, k0);
}

}  // namespace

// directions per walk of the list: 6 = one walk, 3 = two walks (DESIGN.md section 3 has the resource figures of both)
#ifndef MGS_TAN_WALK_DIRS
#define MGS_TAN_WALK_DIRS 6
#endif
constexpr int TAN_WALK_DIRS = MGS_TAN_WALK_DIRS;

}  // namespace mgs

extern "C" size_t mgs_pose_tangent_bytes(int32_t P) {
    return (size_t)(P < 0 ? 0 : P) * mgs::TAN_FLOATS * sizeof(float) + mgs::ScratchCursor::ALIGN;
}

extern "C" int mgs_pose_jacobian(const mgs_camera* cam, int32_t P, uint64_t num_rendered, const float* means3D,
                                 const float* scales, const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                                 const void* geometry, const void* binning, const void* image, void* tangent_scratch, float* J,
                                 void* stream) {
    using namespace mgs;
    if (check_cam(cam, "mgs_pose_jacobian")) return 1;
    if (P < 0) { set_error("mgs_pose_jacobian: P must be >= 0"); return 1; }
    if (check_map_size(P, "mgs_pose_jacobian")) return 1;
    if (cam->sh_coeffs > 0) {
        set_error("mgs_pose_jacobian: the forward used SH colours, which depend on the camera position; only colors_precomp is supported");
        return 1;
    }
    if (!J) { set_error("mgs_pose_jacobian: J must be non-NULL"); return 1; }
    const int W = cam->image_width, H = cam->image_height;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {
        MGS_HIP(hipMemsetAsync(J, 0, (size_t)30 * H * W * sizeof(float), s));
        return 0;
    }
    if (!means3D || !radii || !geometry || !image || !tangent_scratch) {
        set_error("mgs_pose_jacobian: means3D, radii, geometry, image, tangent_scratch must be non-NULL");
        return 1;
    }
    if ((cov3D_precomp != nullptr) == (scales != nullptr || rotations != nullptr) || (!cov3D_precomp && (!scales || !rotations))) {
        set_error("mgs_pose_jacobian: provide exactly one of either scale/rotation pair or precomputed 3D covariance");
        return 1;
    }
    if (num_rendered > 0 && !binning) { set_error("mgs_pose_jacobian: binning scratch is NULL"); return 1; }
    const auto [g, img, b] = carve_forward(geometry, binning, image, P, num_rendered, W, H);
    ScratchCursor cur(tangent_scratch);
    float* tan = cur.take<float>((size_t)P * TAN_FLOATS * sizeof(float));

    TanRecArgs ra;
    ra.means3D = means3D; ra.scales = scales; ra.rotations = rotations; ra.cov3D = cov3D_precomp; ra.radii = radii;
    ra.V = cam->viewmatrix; ra.PM = cam->projmatrix; ra.PR = cam->projmatrix_raw; ra.tan = tan;
    ra.tanfovx = cam->tanfovx; ra.tanfovy = cam->tanfovy;
    ra.focal_x = (float)W / (2.0f * cam->tanfovx); ra.focal_y = (float)H / (2.0f * cam->tanfovy);
    ra.mod = cam->scale_modifier; ra.P = P; ra.W = W; ra.H = H; ra.iso = cam->scale_dim == 1;
    hipLaunchKernelGGL(pose_tangent_records_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, ra);
    MGS_HIP(hipGetLastError());
    const FeatArgs a = make_feat_args(*cam, 0, g, b, img);
    const int ntiles = tiles_x(W) * tiles_y(H);
    hipLaunchKernelGGL(pose_tangent_blend_kernel<TAN_WALK_DIRS>, dim3(ntiles), dim3(256), 0, s, a, (const float*)tan, cam->bg, J);
    MGS_HIP(hipGetLastError());
    return 0;
}
