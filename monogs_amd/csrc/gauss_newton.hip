// Gauss-Newton tracking: the normal equations of the tracking loss's rows from the pose-tangent planes (pose_tangent.hip), and the
// damped step with the SE(3) retraction and camera refresh of mgs_pose_step (se3.h: MGS_SE3_RETRACT, camera_entry).
//
// Boundary replaced: the reference's tracker takes up to 100 Adam steps per frame on the summed gradient
// (/root/reference/utils/slam_tracker.py:142-176, get_loss_tracking at utils/slam_utils.py:58-98); second-order steps need the
// per-pixel rows, which only a forward-mode pass gives.
//
// Unknowns x = (rho, theta, a, b).  Rows ("Pose tangents"):
//   colour  r_c = e^a C_c + b - I_c   where mask grad_mask (O > 0.99)   d/dx = (e^a J[5 k + c], e^a C_c, 1)   scale 0.5 / (3 H W)
//   depth   r_d = D - D_gt            where (D_gt > 0) (O > 0.99)        d/dx = (J[5 k + 3], 0, 0)             scale 1 / N_d
// with the Huber weight omega = 1 if |r| <= delta else delta / |r|, formed in float32; everything else in double from the
// per-pixel product on.  Launch 1: per-workgroup partial sums (block_sum: fixed order), launch 2: one workgroup per output
// adds the partials in a fixed order, applies 1 / N_d and writes the system.  No atomics: bitwise reproducible.
#include "common.h"
#include "se3.h"

namespace mgs {

constexpr int GN_SYS = MGS_GN_SYSTEM_DOUBLES;      // H[8][8], g[8], E, N_rgb, N_d
constexpr int GN_H8 = 36, GN_H6 = 21;              // upper triangles
constexpr int GN_COL = GN_H8 + 8 + 2;              // colour partials: H, g, E, N_rgb
constexpr int GN_DEP = GN_H6 + 6 + 2;              // depth partials: H, g, E, N_d
constexpr int GN_PART = GN_COL + GN_DEP;
constexpr int GN_MAX_BLOCKS = 256;              // one workgroup per compute unit: each runs at one wave per SIMD
static_assert(GN_SYS == 75, "include/monogs_raster.h");

__host__ __device__ inline int gn_upper(int n, int i, int j) { return i * n - i * (i - 1) / 2 + (j - i); }   // i <= j
inline int gn_blocks(int W, int H) {
    const size_t n = ((size_t)W * H + 255) / 256;
    return (int)(n < 1 ? 1 : (n > (size_t)GN_MAX_BLOCKS ? (size_t)GN_MAX_BLOCKS : n));
}

struct GnArgs {
    const float *J, *render, *depth, *opacity, *gt_rgb, *gt_depth, *exp_a, *exp_b;
    const uint8_t *mask, *grad_mask;
    double* part;             // [blocks][GN_PART]
    float delta_rgb, delta_depth;
    int W, H, rgb_only, threads;
};

// omega in float32, the Huber cost in double
__device__ __forceinline__ void gn_huber(double r, float delta, double& omega, double& rho) {
    const float ar = fabsf((float)r);
    if (ar <= delta) {
        omega = 1.0;
        rho = 0.5 * r * r;
    } else {
        omega = (double)(delta / ar);
        rho = (double)delta * (fabs(r) - 0.5 * (double)delta);
    }
}

__global__ void __launch_bounds__(256) gn_normal_partial_kernel(GnArgs a) {
    __shared__ double s_sum[GN_PART][4];
    const size_t HW = (size_t)a.W * a.H;
    const size_t p0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    double* const out = a.part + (size_t)blockIdx.x * GN_PART;
    const double ea = a.exp_a ? exp((double)a.exp_a[0]) : 1.0, eb = a.exp_b ? (double)a.exp_b[0] : 0.0;
    {   // ---- colour rows
        double Hc[GN_H8], gc[8], E = 0.0, N = 0.0;
#pragma unroll
        for (int i = 0; i < GN_H8; ++i) Hc[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) gc[i] = 0.0;
        const double scale = 0.5 / (3.0 * (double)HW);
        for (size_t p = p0; p < HW; p += (size_t)a.threads) {
            if (!(a.opacity[p] > 0.99f) || (a.mask && !a.mask[p]) || !a.grad_mask[p]) continue;
            N += 1.0;
#pragma unroll 1
            for (int c = 0; c < 3; ++c) {
                const double C = (double)a.render[(size_t)c * HW + p];
                const double r = ea * C + eb - (double)a.gt_rgb[(size_t)c * HW + p];
                double jv[8];
#pragma unroll
                for (int k = 0; k < 6; ++k) jv[k] = ea * (double)a.J[(size_t)(5 * k + c) * HW + p];
                jv[6] = ea * C;
                jv[7] = 1.0;
                double omega, rho;
                gn_huber(r, a.delta_rgb, omega, rho);
                const double w = scale * omega;
                E += scale * rho;
                int at = 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const double wi = w * jv[i];
                    gc[i] += wi * r;
#pragma unroll
                    for (int j = i; j < 8; ++j) Hc[at++] += wi * jv[j];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < GN_H8; ++i) Hc[i] = block_sum(Hc[i], s_sum[i]);
#pragma unroll
        for (int i = 0; i < 8; ++i) gc[i] = block_sum(gc[i], s_sum[GN_H8 + i]);
        E = block_sum(E, s_sum[GN_H8 + 8]);
        N = block_sum(N, s_sum[GN_H8 + 9]);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < GN_H8; ++i) out[i] = Hc[i];
#pragma unroll
            for (int i = 0; i < 8; ++i) out[GN_H8 + i] = gc[i];
            out[GN_H8 + 8] = E;
            out[GN_H8 + 9] = N;
        }
    }
    {   // ---- depth rows (unscaled: 1 / N_d is known only to the second launch)
        double Hd[GN_H6], gd[6], E = 0.0, N = 0.0;
#pragma unroll
        for (int i = 0; i < GN_H6; ++i) Hd[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) gd[i] = 0.0;
        if (!a.rgb_only)
            for (size_t p = p0; p < HW; p += (size_t)a.threads) {
                const float dgt = a.gt_depth[p];
                if (!(dgt > 0.f) || !(a.opacity[p] > 0.99f)) continue;
                N += 1.0;
                const double r = (double)a.depth[p] - (double)dgt;
                double jv[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) jv[k] = (double)a.J[(size_t)(5 * k + 3) * HW + p];
                double omega, rho;
                gn_huber(r, a.delta_depth, omega, rho);
                E += rho;
                int at = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const double wi = omega * jv[i];
                    gd[i] += wi * r;
#pragma unroll
                    for (int j = i; j < 6; ++j) Hd[at++] += wi * jv[j];
                }
            }
#pragma unroll
        for (int i = 0; i < GN_H6; ++i) Hd[i] = block_sum(Hd[i], s_sum[GN_COL + i]);
#pragma unroll
        for (int i = 0; i < 6; ++i) gd[i] = block_sum(gd[i], s_sum[GN_COL + GN_H6 + i]);
        E = block_sum(E, s_sum[GN_COL + GN_H6 + 6]);
        N = block_sum(N, s_sum[GN_COL + GN_H6 + 7]);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < GN_H6; ++i) out[GN_COL + i] = Hd[i];
#pragma unroll
            for (int i = 0; i < 6; ++i) out[GN_COL + GN_H6 + i] = gd[i];
            out[GN_COL + GN_H6 + 6] = E;
            out[GN_COL + GN_H6 + 7] = N;
        }
    }
}

// One workgroup per output double t of the system: thread l adds the partial rows l, l + 256, ... of the (at most two) entries that
// make up sys[t] and of N_d, block_sum adds the 256 values; the depth part is scaled by 1 / N_d here.  (One workgroup for all 75
// entries spent ~190 us on 75 dependent trips through the partials.)
__global__ void __launch_bounds__(256) gn_normal_reduce_kernel(const double* __restrict__ part, int nblocks, double* __restrict__ sys) {
    __shared__ double s_c[4], s_d[4], s_n[4];
    const int t = (int)blockIdx.x;
    int ec = -1, ed = -1;                       // partial entries: the colour rows' and the depth rows' share of sys[t]
    if (t < 64) {
        const int i = t >> 3, j = t & 7, lo = i < j ? i : j, hi = i < j ? j : i;
        ec = gn_upper(8, lo, hi);
        if (hi < 6) ed = GN_COL + gn_upper(6, lo, hi);
    } else if (t < 72) {
        ec = GN_H8 + (t - 64);
        if (t - 64 < 6) ed = GN_COL + GN_H6 + (t - 64);
    } else if (t == 72) {
        ec = GN_H8 + 8;
        ed = GN_COL + GN_H6 + 6;
    } else if (t == 73) {
        ec = GN_H8 + 9;
    }
    double vc = 0.0, vd = 0.0, vn = 0.0;
    for (int b = (int)threadIdx.x; b < nblocks; b += 256) {
        const double* row = part + (size_t)b * GN_PART;
        if (ec >= 0) vc += row[ec];
        if (ed >= 0) vd += row[ed];
        vn += row[GN_COL + GN_H6 + 7];
    }
    vc = block_sum(vc, s_c);
    vd = block_sum(vd, s_d);
    vn = block_sum(vn, s_n);
    if (threadIdx.x != 0) return;
    const double inv_d = vn > 0.0 ? 1.0 / vn : 0.0;
    sys[t] = t == 74 ? vn : vc + inv_d * vd;
}

struct GnStepArgs {
    float *R, *T, *exp_a, *exp_b;
    const double* sys;
    float lam, lam_abs, max_rot, max_trans, converged_threshold;
    float* out;               // [4] {converged, |tau|, E, status}
    float* host_flag;
    int flags;
    const float* proj_T;
    float *view_T, *full_T, *campos;
};

// (H + lam diag(H) + lam_abs I) x = -g by Cholesky in double, N = 8 unknowns or the 6 x 6 pose block; every loop unrolled:
// the matrix lives in registers
template <int N>
__device__ __forceinline__ bool gn_solve(const double* __restrict__ sys, double lam, double lam_abs, double x[8]) {
    double L[N][N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) L[i][j] = sys[8 * i + j];
#pragma unroll
    for (int i = 0; i < N; ++i) L[i][i] = L[i][i] + lam * L[i][i] + lam_abs;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && d > 0.0 && d < 1.0e300;          // non-positive, NaN or infinite pivot
        const double dj = sqrt(ok ? d : 1.0);
        L[j][j] = dj;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / dj;
        }
    }
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = -sys[64 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
        ok = ok && fabs(x[i]) < 1.0e300;
    }
#pragma unroll
    for (int i = N; i < 8; ++i) x[i] = 0.0;
    return ok;
}

__global__ void pose_gn_step_kernel(GnStepArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if ((a.flags & MGS_POSE_STICKY) && a.out[0] > 0.5f) {          // as pose_step_one: a replay after convergence is a no-op
        if (a.host_flag) a.host_flag[0] = 1.f;
        return;
    }
    const bool pose_only = (a.flags & MGS_GN_FIX_EXPOSURE) || !a.exp_a || !a.exp_b;
    double x[8];
    const bool ok = pose_only ? gn_solve<6>(a.sys, (double)a.lam, (double)a.lam_abs, x)
                              : gn_solve<8>(a.sys, (double)a.lam, (double)a.lam_abs, x);
    const float E = (float)a.sys[72];
    if (!ok) {
        a.out[0] = 0.f; a.out[1] = 0.f; a.out[2] = E; a.out[3] = 1.f;
        if (a.host_flag) a.host_flag[0] = 0.f;
        return;
    }
    // the whole step scaled so that |theta| <= max_rot and |rho| <= max_trans
    const double nr = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), nt = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
    double sc = 1.0;
    if (nt > (double)a.max_rot) sc = (double)a.max_rot / nt;
    if (nr * sc > (double)a.max_trans) sc = (double)a.max_trans / nr;
    const float rho[3] = {(float)(sc * x[0]), (float)(sc * x[1]), (float)(sc * x[2])};
    const float th[3] = {(float)(sc * x[3]), (float)(sc * x[4]), (float)(sc * x[5])};
    MGS_SE3_RETRACT(th, rho, a.R, a.T);
    if (!pose_only) {
        a.exp_a[0] = a.exp_a[0] + (float)(sc * x[6]);
        a.exp_b[0] = a.exp_b[0] + (float)(sc * x[7]);
    }
    a.out[0] = tn < a.converged_threshold ? 1.f : 0.f;
    a.out[1] = tn;
    a.out[2] = E;
    a.out[3] = 0.f;
    if (a.host_flag) a.host_flag[0] = a.out[0];
    if (a.view_T) {
        float Tn[3];
        for (int i = 0; i < 3; ++i) Tn[i] = a.T[i];
        for (int t = 0; t < 19; ++t) camera_entry(Rn, Tn, a.proj_T, t, a.view_T, a.full_T, a.campos);
    }
}

}  // namespace mgs

extern "C" size_t mgs_gn_scratch_bytes(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    return (size_t)mgs::gn_blocks(width, height) * mgs::GN_PART * sizeof(double);
}

extern "C" int mgs_gn_normal_equations(int32_t width, int32_t height, int32_t mode, const float* J, const float* render,
                                       const float* depth, const float* opacity, const float* gt_rgb, const float* gt_depth,
                                       const uint8_t* mask, const uint8_t* grad_mask, const float* exposure_a,
                                       const float* exposure_b, float delta_rgb, float delta_depth, void* scratch, double* system,
                                       void* stream) {
    using namespace mgs;
    if (width <= 0 || height <= 0) { set_error("mgs_gn_normal_equations: image size must be positive"); return 1; }
    if (mode & ~(MGS_LOSS_TRACKING | MGS_LOSS_RGB_ONLY)) { set_error("mgs_gn_normal_equations: mode is MGS_LOSS_TRACKING, optionally with MGS_LOSS_RGB_ONLY"); return 1; }
    const bool rgb_only = (mode & MGS_LOSS_RGB_ONLY) != 0;
    if (!J || !render || !opacity || !gt_rgb || !grad_mask || !scratch || !system) {
        set_error("mgs_gn_normal_equations: J, render, opacity, gt_rgb, grad_mask, scratch, system must be non-NULL");
        return 1;
    }
    if (!rgb_only && (!depth || !gt_depth)) { set_error("mgs_gn_normal_equations: depth and gt_depth must be non-NULL without MGS_LOSS_RGB_ONLY"); return 1; }
    if ((exposure_a == nullptr) != (exposure_b == nullptr)) { set_error("mgs_gn_normal_equations: exposure_a and exposure_b go together"); return 1; }
    if (!(delta_rgb > 0.f) || !(delta_depth > 0.f)) { set_error("mgs_gn_normal_equations: delta_rgb and delta_depth must be positive"); return 1; }
    if ((size_t)scratch % 8 != 0 || (size_t)system % 8 != 0) { set_error("mgs_gn_normal_equations: scratch and system must be 8-byte aligned"); return 1; }
    GnArgs a;
    a.J = J; a.render = render; a.depth = depth; a.opacity = opacity; a.gt_rgb = gt_rgb; a.gt_depth = gt_depth;
    a.exp_a = exposure_a; a.exp_b = exposure_b; a.mask = mask; a.grad_mask = grad_mask; a.part = (double*)scratch;
    a.delta_rgb = delta_rgb; a.delta_depth = delta_depth; a.W = width; a.H = height; a.rgb_only = rgb_only ? 1 : 0;
    const int nb = gn_blocks(width, height);
    a.threads = nb * 256;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_normal_partial_kernel, dim3(nb), dim3(256), 0, s, a);
    MGS_HIP(hipGetLastError());
    hipLaunchKernelGGL(gn_normal_reduce_kernel, dim3(GN_SYS), dim3(256), 0, s, (const double*)scratch, nb, system);
    MGS_HIP(hipGetLastError());
    return 0;
}

extern "C" int mgs_pose_gn_step(float* R, float* T, float* exposure_a, float* exposure_b, const double* system, float lam,
                                float lam_abs, float max_rot, float max_trans, float converged_threshold, float* out,
                                int32_t flags, float* host_flag, const float* projmatrix_raw, float* viewmatrix,
                                float* projmatrix, float* campos, void* stream) {
    using namespace mgs;
    if (!R || !T || !system || !out) { set_error("mgs_pose_gn_step: R, T, system, out must be non-NULL"); return 1; }
    if ((exposure_a == nullptr) != (exposure_b == nullptr)) { set_error("mgs_pose_gn_step: exposure_a and exposure_b go together"); return 1; }
    if (!(lam >= 0.f) || !(lam_abs >= 0.f) || !(max_rot > 0.f) || !(max_trans > 0.f)) {
        set_error("mgs_pose_gn_step: lam, lam_abs must be >= 0 and max_rot, max_trans positive");
        return 1;
    }
    if (flags & ~(MGS_POSE_STICKY | MGS_GN_FIX_EXPOSURE)) { set_error("mgs_pose_gn_step: unknown flag"); return 1; }
    if (viewmatrix && (!projmatrix_raw || !projmatrix || !campos)) {
        set_error("mgs_pose_gn_step: camera refresh needs projmatrix_raw, viewmatrix, projmatrix and campos");
        return 1;
    }
    GnStepArgs a;
    a.R = R; a.T = T; a.exp_a = exposure_a; a.exp_b = exposure_b; a.sys = system; a.lam = lam; a.lam_abs = lam_abs;
    a.max_rot = max_rot; a.max_trans = max_trans; a.converged_threshold = converged_threshold; a.out = out;
    a.host_flag = host_flag; a.flags = flags; a.proj_T = projmatrix_raw; a.view_T = viewmatrix; a.full_T = projmatrix;
    a.campos = campos;
    hipLaunchKernelGGL(pose_gn_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    MGS_HIP(hipGetLastError());
    return 0;
}
