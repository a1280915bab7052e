// SE(3) pose arithmetic shared by the pose units: the camera matrices of a viewpoint and the retraction of a pose update
// (pose.hip: the Adam step; gauss_newton.hip: the Gauss-Newton step).
#pragma once

#include "common.h"

namespace mgs {

__device__ __forceinline__ void mat3mul(const float* A, const float* B, float* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// Camera matrices of one viewpoint in ONE launch: what the reference assembles per render() from R, T with
// getWorld2View + transpose, a 4x4 bmm and a 4x4 inverse
// (/root/reference/gaussian_splatting/utils/graphics_utils.py:33-42, /root/reference/utils/camera_utils.py:171-178,
// /root/reference/gaussian_splatting/gaussian_renderer/__init__.py:61-68) -- about ten small kernels in PyTorch.
// All matrices are the TRANSPOSED (row-vector) ones the rasteriser takes.
// Entry t of the 35 outputs (16 view, 16 full projection, 3 camera centre), with the products contracted explicitly:
// camera_setup_kernel (one thread per entry) and pose_step_kernel (its one thread, all entries) give the same bits.
__device__ __forceinline__ void camera_entry(const float* R, const float* T, const float* proj_T, int t, float* view_T,
                                             float* full_T, float* campos) {
    auto vT = [&](int i, int k) -> float {          // view_T[i][k] = W2C[k][i],  W2C = [[R, t], [0, 1]]
        if (k < 3) return i < 3 ? R[3 * k + i] : T[k];
        return i == 3 ? 1.f : 0.f;
    };
    if (t < 16) {
        const int i = t >> 2, j = t & 3;
        view_T[t] = vT(i, j);
        float acc = 0.f;
        for (int k = 0; k < 4; ++k) acc = __builtin_fmaf(vT(i, k), proj_T[4 * k + j], acc);
        full_T[t] = acc;
    } else if (t < 19) {
        const int i = t - 16;                       // camera centre -R^T t
        campos[i] = -__builtin_fmaf(R[6 + i], T[2], __builtin_fmaf(R[3 + i], T[1], R[i] * T[0]));
    }
}

// The retraction of every pose update of the library, stated once (pose.hip's pose_step_one, gauss_newton.hip's step):  T_cw <- exp(tau^) T_cw,
// tau = [rho; theta]  (/root/reference/utils/pose_utils.py:25-93).  `th`, `rho`: float[3]; `R`, `T`: the pose, updated in place; declares
// Rn[9], the new R, and tn = |tau|.  A macro, not a function: written in place the statements give pose_step_kernel the parent's
// machine code instruction for instruction, as a helper they come out with another register assignment (tools/kernel_identity.py).
#define MGS_SE3_RETRACT(th, rho, R, T)                                                                                  \
    const float W[9] = {0.f, -th[2], th[1], th[2], 0.f, -th[0], -th[1], th[0], 0.f};                                    \
    float W2[9];                                                                                                        \
    mat3mul(W, W, W2);                                                                                                  \
    const float angle = sqrtf(th[0] * th[0] + th[1] * th[1] + th[2] * th[2]);                                           \
    float ca, cb, va, vb;   /* R = I + ca W + cb W2 ; V = I + va W + vb W2 */                                           \
    if (angle < 1e-5f) {                                                                                                \
        ca = 1.f; cb = 0.5f; va = 0.5f; vb = 1.f / 6.f;                                                                 \
    } else {                                                                                                            \
        const float s = sinf(angle), c = cosf(angle), a2 = angle * angle;                                               \
        ca = s / angle; cb = (1.f - c) / a2; va = (1.f - c) / a2; vb = (angle - s) / (a2 * angle);                      \
    }                                                                                                                   \
    float dR[9], V[9];                                                                                                  \
    for (int i = 0; i < 9; ++i) {                                                                                       \
        const float eye = (i % 4 == 0) ? 1.f : 0.f;                                                                     \
        dR[i] = eye + ca * W[i] + cb * W2[i];                                                                           \
        V[i] = eye + va * W[i] + vb * W2[i];                                                                            \
    }                                                                                                                   \
    float dt[3];                                                                                                        \
    for (int i = 0; i < 3; ++i) dt[i] = V[3 * i] * rho[0] + V[3 * i + 1] * rho[1] + V[3 * i + 2] * rho[2];              \
    float Rn[9], Ro[9], To[3];                                                                                          \
    for (int i = 0; i < 9; ++i) Ro[i] = (R)[i];                                                                         \
    for (int i = 0; i < 3; ++i) To[i] = (T)[i];                                                                         \
    mat3mul(dR, Ro, Rn);                                                                                                \
    for (int i = 0; i < 9; ++i) (R)[i] = Rn[i];                                                                         \
    for (int i = 0; i < 3; ++i) (T)[i] = dR[3 * i] * To[0] + dR[3 * i + 1] * To[1] + dR[3 * i + 2] * To[2] + dt[i];     \
    const float tn = sqrtf(rho[0] * rho[0] + rho[1] * rho[1] + rho[2] * rho[2] + angle * angle)

}  // namespace mgs
