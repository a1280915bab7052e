// Fused pose update of the tracking / mapping loops: Adam step on (cam_rot_delta, cam_trans_delta,
// exposure_a, exposure_b) followed by the SE(3) retraction  T_cw <- exp([rho; theta]^) T_cw  and the reset
// of the deltas -- what the reference does with torch.optim.Adam.step() plus utils/pose_utils.py:76-93
// (`update_pose`) in ~60 tiny launches and one host sync per iteration.  One single-wave kernel here.
// Caller-side widening (optimiser step next to the rasteriser backward).
#include "common.h"
#include "se3.h"             // mat3mul, camera_entry, MGS_SE3_RETRACT: shared with gauss_newton.hip

namespace mgs {

struct PoseStepArgs {
    float* R;             // [3,3] row-major world->camera rotation, updated in place
    float* T;             // [3]
    float* rot_delta;     // [3] parameter (zero on entry, zero on exit)
    float* trans_delta;   // [3]
    float* exp_a;         // [1] parameter, updated in place (may be NULL)
    float* exp_b;         // [1]
    const float* g_rot;   // gradients (NULL = zero)
    const float* g_trans;
    const float* g_a;
    const float* g_b;
    float* m;             // [8] Adam first moments: rot(3) trans(3) a b
    float* v;             // [8] Adam second moments
    float* out;           // [2] {converged (0/1), |tau|}
    float* host_flag;     // optional: a device-visible HOST word (pinned memory) that receives out[0] as well, so that a loop
                          // replayed from a hipGraph needs no device-to-host copy (a ~4 us blit kernel) per iteration
    float lr_rot, lr_trans, lr_exp, beta1, beta2, eps, converged_threshold;
    int step;             // 1-based Adam step count of this update (used when step_dev is NULL)
    int* step_dev;        // optional device counter: incremented here, so a captured graph replays correctly
    int flags;            // MGS_POSE_STICKY: once out[0] says converged, later calls change nothing
    // optional: the camera tensors of this viewpoint, recomputed from the new R, T right here -- the next render of a loop
    // then needs no camera_setup launch (the two kernels share camera_entry: same bits)
    const float* proj_T;
    float *view_T, *full_T, *campos;
};

__global__ void camera_setup_kernel(const float* __restrict__ R, const float* __restrict__ T,
                                    const float* __restrict__ proj_T, float* __restrict__ view_T,
                                    float* __restrict__ full_T, float* __restrict__ campos) {
    camera_entry(R, T, proj_T, (int)threadIdx.x, view_T, full_T, campos);
}

__device__ __forceinline__ void pose_step_one(const PoseStepArgs& a) {
    // Sticky convergence: the reference's tracker leaves its loop at the first converged update
    // (/root/reference/utils/slam_tracker.py:172-176).  With the loop replayed from a hipGraph the host learns of the
    // convergence one replay late; making that extra replay a no-op keeps the result identical to the early exit.
    if ((a.flags & 1) && a.out[0] > 0.5f) {
        if (a.host_flag) a.host_flag[0] = 1.f;
        return;
    }
    // ---- Adam (torch.optim.Adam defaults: no weight decay, no amsgrad), one scalar at a time
    int step = a.step;
    if (a.step_dev) { step = a.step_dev[0] + 1; a.step_dev[0] = step; }
    const float bc1 = 1.f - powf(a.beta1, (float)step), bc2 = 1.f - powf(a.beta2, (float)step);
    float p[8], g[8];
    for (int i = 0; i < 3; ++i) {
        p[i] = a.rot_delta[i];     g[i] = a.g_rot ? a.g_rot[i] : 0.f;
        p[3 + i] = a.trans_delta[i]; g[3 + i] = a.g_trans ? a.g_trans[i] : 0.f;
    }
    p[6] = a.exp_a ? a.exp_a[0] : 0.f; g[6] = a.g_a ? a.g_a[0] : 0.f;
    p[7] = a.exp_b ? a.exp_b[0] : 0.f; g[7] = a.g_b ? a.g_b[0] : 0.f;
    for (int i = 0; i < 8; ++i) {
        const float lr = i < 3 ? a.lr_rot : (i < 6 ? a.lr_trans : a.lr_exp);
        const float m = a.beta1 * a.m[i] + (1.f - a.beta1) * g[i];
        const float v = a.beta2 * a.v[i] + (1.f - a.beta2) * g[i] * g[i];
        a.m[i] = m; a.v[i] = v;
        const float denom = sqrtf(v) / sqrtf(bc2) + a.eps;
        p[i] = p[i] - (lr / bc1) * (m / denom);
    }
    if (a.exp_a) a.exp_a[0] = p[6];
    if (a.exp_b) a.exp_b[0] = p[7];
    // ---- tau = [rho; theta];  T <- exp(tau^) T
    const float th[3] = {p[0], p[1], p[2]}, rho[3] = {p[3], p[4], p[5]};
    MGS_SE3_RETRACT(th, rho, a.R, a.T);
    a.out[0] = tn < a.converged_threshold ? 1.f : 0.f;
    a.out[1] = tn;
    if (a.host_flag) a.host_flag[0] = a.out[0];
    for (int i = 0; i < 3; ++i) { a.rot_delta[i] = 0.f; a.trans_delta[i] = 0.f; }
    if (a.view_T) {
        float Tn[3];
        for (int i = 0; i < 3; ++i) Tn[i] = a.T[i];
        for (int t = 0; t < 19; ++t) camera_entry(Rn, Tn, a.proj_T, t, a.view_T, a.full_T, a.campos);
    }
}

__global__ void pose_step_kernel(PoseStepArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    pose_step_one(a);
}

// The pose steps of ALL the keyframes of a mapping window in one launch (one workgroup each; they are independent): a window
// of eight used to end its iteration with seven dependent 7-us launches.
constexpr int POSE_BATCH_MAX = 16;
struct PoseBatchArgs { PoseStepArgs v[POSE_BATCH_MAX]; };
__global__ void pose_step_batch_kernel(PoseBatchArgs b) {
    if (threadIdx.x != 0) return;
    pose_step_one(b.v[blockIdx.x]);
}

}  // namespace mgs

using namespace mgs;

extern "C" int mgs_camera_setup(const float* R, const float* T, const float* projmatrix_raw, float* viewmatrix,
                                float* projmatrix, float* campos, void* stream) {
    if (!R || !T || !projmatrix_raw || !viewmatrix || !projmatrix || !campos) { set_error("mgs_camera_setup: NULL argument"); return 1; }
    hipLaunchKernelGGL(camera_setup_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, R, T, projmatrix_raw, viewmatrix,
                       projmatrix, campos);
    MGS_HIP(hipGetLastError());
    return 0;
}

static int fill_pose_args(PoseStepArgs& a, float* R, float* T, float* rot_delta, float* trans_delta, float* exposure_a,
                          float* exposure_b, const float* grad_rot, const float* grad_trans, const float* grad_a,
                          const float* grad_b, float* adam_m, float* adam_v, int32_t step, float lr_rot, float lr_trans,
                          float lr_exposure, float beta1, float beta2, float eps, float converged_threshold,
                          int32_t* step_counter, float* out, int32_t flags, float* host_flag, const float* projmatrix_raw,
                          float* viewmatrix, float* projmatrix, float* campos) {
    if (!R || !T || !rot_delta || !trans_delta || !adam_m || !adam_v || !out) {
        set_error("R, T, rot_delta, trans_delta, adam_m, adam_v, out must be non-NULL");
        return 1;
    }
    if (!step_counter && step < 1) { set_error("step is 1-based"); return 1; }
    if (viewmatrix && (!projmatrix_raw || !projmatrix || !campos)) {
        set_error("camera refresh needs projmatrix_raw, viewmatrix, projmatrix and campos");
        return 1;
    }
    a.R = R; a.T = T; a.rot_delta = rot_delta; a.trans_delta = trans_delta; a.exp_a = exposure_a; a.exp_b = exposure_b;
    a.g_rot = grad_rot; a.g_trans = grad_trans; a.g_a = grad_a; a.g_b = grad_b; a.m = adam_m; a.v = adam_v; a.out = out;
    a.lr_rot = lr_rot; a.lr_trans = lr_trans; a.lr_exp = lr_exposure; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    a.converged_threshold = converged_threshold; a.step = step; a.step_dev = step_counter; a.flags = flags; a.host_flag = host_flag;
    a.proj_T = projmatrix_raw; a.view_T = viewmatrix; a.full_T = projmatrix; a.campos = campos;
    return 0;
}

extern "C" int mgs_pose_step(float* R, float* T, float* rot_delta, float* trans_delta, float* exposure_a,
                             float* exposure_b, const float* grad_rot, const float* grad_trans, const float* grad_a,
                             const float* grad_b, float* adam_m, float* adam_v, int32_t step, float lr_rot,
                             float lr_trans, float lr_exposure, float beta1, float beta2, float eps,
                             float converged_threshold, int32_t* step_counter, float* out, int32_t flags,
                             float* host_flag, const float* projmatrix_raw, float* viewmatrix, float* projmatrix,
                             float* campos, void* stream) {
    PoseStepArgs a;
    if (fill_pose_args(a, R, T, rot_delta, trans_delta, exposure_a, exposure_b, grad_rot, grad_trans, grad_a, grad_b, adam_m,
                       adam_v, step, lr_rot, lr_trans, lr_exposure, beta1, beta2, eps, converged_threshold, step_counter, out,
                       flags, host_flag, projmatrix_raw, viewmatrix, projmatrix, campos)) return 1;
    hipLaunchKernelGGL(pose_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    MGS_HIP(hipGetLastError());
    return 0;
}

// n <= 16 independent pose steps in one launch.  `ptrs` is a HOST array of n x 18 device pointers in the order of
// mgs_pose_step's pointer arguments: R, T, rot_delta, trans_delta, exposure_a, exposure_b, grad_rot, grad_trans, grad_a,
// grad_b, adam_m, adam_v, step_counter, out, projmatrix_raw, viewmatrix, projmatrix, campos (NULL where optional).
// The scalars are shared by the batch (the keyframes of a window use the same learning rates).
extern "C" int mgs_pose_step_batch(int32_t n, void* const* ptrs, float lr_rot, float lr_trans, float lr_exposure, float beta1,
                                   float beta2, float eps, float converged_threshold, int32_t flags, void* stream) {
    if (n < 0 || n > POSE_BATCH_MAX || (n > 0 && !ptrs)) { set_error("mgs_pose_step_batch: 0..16 poses"); return 1; }
    if (n == 0) return 0;
    PoseBatchArgs b;
    for (int i = 0; i < n; ++i) {
        void* const* q = ptrs + (size_t)i * 18;
        if (!q[12]) { set_error("mgs_pose_step_batch needs device step counters"); return 1; }
        if (fill_pose_args(b.v[i], (float*)q[0], (float*)q[1], (float*)q[2], (float*)q[3], (float*)q[4], (float*)q[5],
                           (const float*)q[6], (const float*)q[7], (const float*)q[8], (const float*)q[9], (float*)q[10],
                           (float*)q[11], 0, lr_rot, lr_trans, lr_exposure, beta1, beta2, eps, converged_threshold,
                           (int32_t*)q[12], (float*)q[13], flags, nullptr, (const float*)q[14], (float*)q[15], (float*)q[16],
                           (float*)q[17])) return 1;
    }
    for (int i = n; i < POSE_BATCH_MAX; ++i) b.v[i] = b.v[0];
    hipLaunchKernelGGL(pose_step_batch_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, b);
    MGS_HIP(hipGetLastError());
    return 0;
}
