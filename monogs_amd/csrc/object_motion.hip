// Rigid object motion ("Object motion"; tests/object_motion_mirror.py restates it in float64): the Gaussians of up to
// MGS_MAX_MOVING_OBJECTS objects moved by one world-frame SE(3) pose each, and the gradient of that reduced to one se(3) tangent per
// object.  Kernels and entry points; the poses are the ones mgs_pose_step_batch (pose.hip) steps.  The reference moves nothing: its
// configs only name the dynamic ids.
//
//   forward   one workgroup of 256 threads per 1024 Gaussians, four per thread 256 apart (coalesced): label -> slot through the
//             256-entry table staged in LDS beside the poses; a moved Gaussian gets x' = R x + t as three fma per component and
//             q' = quat(R) (x) q, every other one is copied bit for bit
//   backward  the same walk: grad_means = R^T g, grad_rots = conj(quat(R)) (x) gq, and the six terms of the object's tangent
//             (g, x' x g + the quaternion's part).  A lane carries the terms of its four Gaussians while they belong to one slot; the
//             wave empties its carries into its own LDS rows when a lane meets another slot, and at the end: a ballot finds the
//             slots held (none: nothing to add); ONE slot: the butterfly (wave_sum); several: every (slot, term) pair is added by a
//             lane of its own over the 64 carries in lane order, from LDS.  After one barrier
//             the four waves' rows are added as block_sum adds them, ((w0 + w1) + (w2 + w3)), and written as the workgroup's row
//             of partials -- zeros included, the scratch is never cleared
//   final     one wave per object: wave_sum_rows over the workgroups' rows
// No float atomics anywhere: the [M,6] result is a function of the inputs alone, bit for bit.  quat(R) is computed per workgroup by
// M lanes in float64 (Shepperd's branches) and rounded once: 16 square roots against 1024 Gaussians' traffic.
// Streaming kernels: 29 + 28 bytes per Gaussian forward (label, mean and quaternion in and out), 1 + 4 x 28 backward.
#include "common.h"

namespace mgs {

constexpr int OM_THREADS = 256;
constexpr int OM_PER_THREAD = 4;
constexpr int OM_ITEMS = OM_THREADS * OM_PER_THREAD;      // Gaussians per workgroup
constexpr int OM_MAX = MGS_MAX_MOVING_OBJECTS;

inline int om_blocks(int P) { return (int)(((size_t)P + OM_ITEMS - 1) / OM_ITEMS); }

struct ObjectPosesLds {
    int slot[256];              // slot of a label, -1: static
    float R[OM_MAX * 9];
    float T[OM_MAX * 3];
    float q[OM_MAX * 4];        // quat(R), (r, x, y, z)
};

// the table and the M poses into LDS (blockDim.x == 256 == the table); ends with the workgroup's barrier
__device__ __forceinline__ void om_stage_poses(ObjectPosesLds& s, int M, const int32_t* __restrict__ slot_of_label,
                                               const float* __restrict__ R, const float* __restrict__ T) {
    const int t = threadIdx.x;
    const int sl = slot_of_label[t];
    s.slot[t] = (sl >= 0 && sl < M) ? sl : -1;
    if (t < M * 9) s.R[t] = R[t];
    if (T && t < M * 3) s.T[t] = T[t];
    if (t < M) {
        const float* r = R + t * 9;
        const double m00 = r[0], m01 = r[1], m02 = r[2], m10 = r[3], m11 = r[4], m12 = r[5], m20 = r[6], m21 = r[7], m22 = r[8];
        const double tr = m00 + m11 + m22;
        double w, x, y, z;
        if (tr > 0.0) {
            const double d = sqrt(tr + 1.0) * 2.0;
            w = 0.25 * d; x = (m21 - m12) / d; y = (m02 - m20) / d; z = (m10 - m01) / d;
        } else if (m00 > m11 && m00 > m22) {
            const double d = sqrt(1.0 + m00 - m11 - m22) * 2.0;
            w = (m21 - m12) / d; x = 0.25 * d; y = (m01 + m10) / d; z = (m02 + m20) / d;
        } else if (m11 > m22) {
            const double d = sqrt(1.0 + m11 - m00 - m22) * 2.0;
            w = (m02 - m20) / d; x = (m01 + m10) / d; y = 0.25 * d; z = (m12 + m21) / d;
        } else {
            const double d = sqrt(1.0 + m22 - m00 - m11) * 2.0;
            w = (m10 - m01) / d; x = (m02 + m20) / d; y = (m12 + m21) / d; z = 0.25 * d;
        }
        s.q[4 * t] = (float)w; s.q[4 * t + 1] = (float)x; s.q[4 * t + 2] = (float)y; s.q[4 * t + 3] = (float)z;
    }
    __syncthreads();
}

// a (x) b, Hamilton, (r, x, y, z): one fma chain per component
__device__ __forceinline__ float4 om_quat_mul(float aw, float ax, float ay, float az, const float4& b) {
    float4 o;
    o.x = fmaf(-az, b.w, fmaf(-ay, b.z, fmaf(-ax, b.y, aw * b.x)));
    o.y = fmaf(-az, b.z, fmaf(ay, b.w, fmaf(ax, b.x, aw * b.y)));
    o.z = fmaf(az, b.y, fmaf(ay, b.x, fmaf(-ax, b.w, aw * b.z)));
    o.w = fmaf(az, b.x, fmaf(-ay, b.y, fmaf(ax, b.z, aw * b.w)));
    return o;
}

__global__ void __launch_bounds__(OM_THREADS)
object_transform_forward_kernel(int P, int M, const uint8_t* __restrict__ labels, const int32_t* __restrict__ slot_of_label,
                                const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ means,
                                const float4* __restrict__ rots, float* __restrict__ means_out, float4* __restrict__ rots_out) {
    __shared__ ObjectPosesLds s;
    om_stage_poses(s, M, slot_of_label, R, T);
    const size_t base = (size_t)blockIdx.x * OM_ITEMS + threadIdx.x;
#pragma unroll
    for (int j = 0; j < OM_PER_THREAD; ++j) {
        const size_t i = base + (size_t)j * OM_THREADS;
        if (i >= (size_t)P) break;
        const int m = s.slot[labels[i]];
        float x = means[3 * i], y = means[3 * i + 1], z = means[3 * i + 2];
        float4 q = rots ? rots[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (m >= 0) {
            const float* r = s.R + 9 * m;
            const float* t = s.T + 3 * m;
            const float nx = fmaf(r[2], z, fmaf(r[1], y, fmaf(r[0], x, t[0])));
            const float ny = fmaf(r[5], z, fmaf(r[4], y, fmaf(r[3], x, t[1])));
            const float nz = fmaf(r[8], z, fmaf(r[7], y, fmaf(r[6], x, t[2])));
            x = nx; y = ny; z = nz;
            const float* a = s.q + 4 * m;
            q = om_quat_mul(a[0], a[1], a[2], a[3], q);
        }
        means_out[3 * i] = x; means_out[3 * i + 1] = y; means_out[3 * i + 2] = z;
        if (rots_out) rots_out[i] = q;
    }
}

__global__ void __launch_bounds__(OM_THREADS)
object_transform_backward_kernel(int P, int M, const uint8_t* __restrict__ labels, const int32_t* __restrict__ slot_of_label,
                                 const float* __restrict__ R, const float* __restrict__ means_out,
                                 const float4* __restrict__ rots_out, const float* __restrict__ g_means_out,
                                 const float4* __restrict__ g_rots_out, float* __restrict__ g_means, float4* __restrict__ g_rots,
                                 float* __restrict__ partials) {
    __shared__ ObjectPosesLds s;
    __shared__ float s_part[OM_THREADS / 64][OM_MAX][6];      // a wave's totals per slot
    __shared__ float s_term[OM_THREADS / 64][64 * 7];         // the serial path: a wave's 64 carries, 7 floats apart (no bank conflict)
    __shared__ int s_slot[OM_THREADS / 64][64];
    for (int e = threadIdx.x; e < (OM_THREADS / 64) * OM_MAX * 6; e += OM_THREADS) (&s_part[0][0][0])[e] = 0.f;
    om_stage_poses(s, M, slot_of_label, R, nullptr);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int grp = lane / 6, kk = lane - 6 * grp;            // serial path: lane (grp, kk) owns term kk of slot 10 pass + grp (grp 10: idle)
    // A lane CARRIES the terms of its Gaussians while they belong to one slot (sl); the wave adds its carries into s_part when a
    // lane meets another slot, and at the end.  One slot among the 64 carries: the butterfly.  Several: every (slot, term) pair
    // is added by its own lane over the 64 carries in lane order.  Which path runs depends on the labels alone.
    int sl = -1;
    float carry[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto flush = [&]() {
        const unsigned long long held = __builtin_amdgcn_ballot_w64(sl >= 0);
        if (held == 0ull) return;                             // no lane of this wave holds a slot: nothing to add
        const int first = (int)bcast((uint32_t)sl, __builtin_ctzll(held));        // wave-uniform
        if (__builtin_amdgcn_ballot_w64(sl == first) == held) {
            float v[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) v[k] = wave_sum(sl >= 0 ? carry[k] : 0.f);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 6; ++k) s_part[wv][first][k] += v[k];
            }
        } else {
            __builtin_amdgcn_wave_barrier();
            s_slot[wv][lane] = sl;
#pragma unroll
            for (int k = 0; k < 6; ++k) s_term[wv][7 * lane + k] = carry[k];
            __builtin_amdgcn_wave_barrier();
            for (int pass = 0; pass * 10 < M; ++pass) {
                if (__builtin_amdgcn_ballot_w64(sl >= pass * 10 && sl < pass * 10 + 10) == 0ull) continue;      // wave-uniform
                const int mine = grp < 10 ? pass * 10 + grp : -2;
                float acc = 0.f;
                for (int j0 = 0; j0 < 64; j0 += 8) {          // eight carries' loads in flight, then their adds in lane order
                    int sj[8];
                    float tj[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { sj[u] = s_slot[wv][j0 + u]; tj[u] = s_term[wv][7 * (j0 + u) + kk]; }
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc += sj[u] == mine ? tj[u] : 0.f;
                }
                if (mine >= 0 && mine < M) s_part[wv][mine][kk] += acc;
            }
            __builtin_amdgcn_wave_barrier();
        }
        sl = -1;
#pragma unroll
        for (int k = 0; k < 6; ++k) carry[k] = 0.f;
    };
    const size_t base = (size_t)blockIdx.x * OM_ITEMS + threadIdx.x;
#pragma unroll 1
    for (int j = 0; j < OM_PER_THREAD; ++j) {
        const size_t i = base + (size_t)j * OM_THREADS;
        int m = -1;
        float c[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (i < (size_t)P) {
            m = s.slot[labels[i]];
            float gx = g_means_out[3 * i], gy = g_means_out[3 * i + 1], gz = g_means_out[3 * i + 2];
            float4 gq = g_rots_out ? g_rots_out[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (m >= 0) {
                const float px = means_out[3 * i], py = means_out[3 * i + 1], pz = means_out[3 * i + 2];
                c[0] = gx; c[1] = gy; c[2] = gz;
                c[3] = fmaf(py, gz, -(pz * gy));
                c[4] = fmaf(pz, gx, -(px * gz));
                c[5] = fmaf(px, gy, -(py * gx));
                if (g_rots_out) {          // q' = (w, v): 1/2 (w gq_v - gq_w v + v x gq_v)
                    const float4 q = rots_out[i];
                    const float w = q.x, vx = q.y, vy = q.z, vz = q.w;
                    c[3] += 0.5f * fmaf(vy, gq.w, fmaf(-vz, gq.z, fmaf(-gq.x, vx, w * gq.y)));
                    c[4] += 0.5f * fmaf(vz, gq.y, fmaf(-vx, gq.w, fmaf(-gq.x, vy, w * gq.z)));
                    c[5] += 0.5f * fmaf(vx, gq.z, fmaf(-vy, gq.y, fmaf(-gq.x, vz, w * gq.w)));
                }
                const float* r = s.R + 9 * m;          // R^T g
                const float nx = fmaf(r[6], gz, fmaf(r[3], gy, r[0] * gx));
                const float ny = fmaf(r[7], gz, fmaf(r[4], gy, r[1] * gx));
                const float nz = fmaf(r[8], gz, fmaf(r[5], gy, r[2] * gx));
                gx = nx; gy = ny; gz = nz;
                const float* a = s.q + 4 * m;
                gq = om_quat_mul(a[0], -a[1], -a[2], -a[3], gq);
            }
            if (g_means) { g_means[3 * i] = gx; g_means[3 * i + 1] = gy; g_means[3 * i + 2] = gz; }
            if (g_rots) g_rots[i] = gq;
        }
        if (__builtin_amdgcn_ballot_w64(m >= 0 && sl >= 0 && sl != m) != 0ull) flush();      // some lane changes slot: the wave empties its carries
        if (m >= 0) {
            sl = m;
#pragma unroll
            for (int k = 0; k < 6; ++k) carry[k] += c[k];
        }
    }
    flush();
    __syncthreads();
    const int t = threadIdx.x;
    if (t < M * 6) {
        const int m = t / 6, k = t - 6 * m;
        partials[(size_t)blockIdx.x * (M * 6) + t] = (s_part[0][m][k] + s_part[1][m][k]) + (s_part[2][m][k] + s_part[3][m][k]);
    }
}

// one wave per object: the workgroups' rows in a fixed order
__global__ void __launch_bounds__(64)
object_tau_final_kernel(int M, int nrows, const float* __restrict__ partials, float* __restrict__ grad_tau) {
    const int m = blockIdx.x, lane = threadIdx.x;
    float v[6];
    wave_sum_rows<6>(partials + 6 * m, (size_t)M * 6, nrows, lane, v);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) grad_tau[6 * m + k] = v[k];
    }
}

}  // namespace mgs

extern "C" size_t mgs_object_motion_scratch_bytes(int32_t P, int32_t M) {
    if (P < 0 || M < 0 || M > mgs::OM_MAX) return 256;
    const size_t rows = (size_t)mgs::om_blocks(P);
    return mgs::align_up((rows ? rows : 1) * (size_t)(M ? M : 1) * 6 * sizeof(float), 256);
}

extern "C" int mgs_object_transform_forward(int32_t P, int32_t M, const uint8_t* labels, const int32_t* slot_of_label, const float* R,
                                            const float* T, const float* means, const float* rots, float* means_out, float* rots_out,
                                            void* stream) {
    using namespace mgs;
    if (P < 0 || M < 0 || M > OM_MAX) { set_error("mgs_object_transform_forward: P >= 0 and 0..%d moving objects (got P = %d, M = %d)", OM_MAX, P, M); return 1; }
    if (!slot_of_label) { set_error("mgs_object_transform_forward: slot_of_label is NULL"); return 1; }
    if (M > 0 && (!R || !T)) { set_error("mgs_object_transform_forward: R and T must be non-NULL when M > 0"); return 1; }
    if (P > 0 && (!labels || !means || !means_out)) { set_error("mgs_object_transform_forward: labels, means, means_out must be non-NULL"); return 1; }
    if ((rots == nullptr) != (rots_out == nullptr)) { set_error("mgs_object_transform_forward: rots and rots_out go together"); return 1; }
    if (P == 0) return 0;
    hipLaunchKernelGGL(object_transform_forward_kernel, dim3((unsigned)om_blocks(P)), dim3(OM_THREADS), 0, (hipStream_t)stream, P, M,
                       labels, slot_of_label, R, T, means, (const float4*)rots, means_out, (float4*)rots_out);
    MGS_HIP(hipGetLastError());
    return 0;
}

extern "C" int mgs_object_transform_backward(int32_t P, int32_t M, const uint8_t* labels, const int32_t* slot_of_label, const float* R,
                                             const float* means_out, const float* rots_out, const float* grad_means_out,
                                             const float* grad_rots_out, float* grad_means, float* grad_rots, float* grad_tau,
                                             void* scratch, void* stream) {
    using namespace mgs;
    if (P < 0 || M < 0 || M > OM_MAX) { set_error("mgs_object_transform_backward: P >= 0 and 0..%d moving objects (got P = %d, M = %d)", OM_MAX, P, M); return 1; }
    if (!slot_of_label) { set_error("mgs_object_transform_backward: slot_of_label is NULL"); return 1; }
    if (M > 0 && (!R || !grad_tau || !scratch)) { set_error("mgs_object_transform_backward: R, grad_tau and scratch must be non-NULL when M > 0"); return 1; }
    if (P > 0 && (!labels || !means_out || !grad_means_out)) { set_error("mgs_object_transform_backward: labels, means_out, grad_means_out must be non-NULL"); return 1; }
    if ((rots_out == nullptr) != (grad_rots_out == nullptr)) { set_error("mgs_object_transform_backward: rots_out and grad_rots_out go together"); return 1; }
    if (grad_rots && !grad_rots_out) { set_error("mgs_object_transform_backward: grad_rots needs grad_rots_out"); return 1; }
    const int rows = om_blocks(P);
    if (P > 0 && (M > 0 || grad_means || grad_rots)) {
        hipLaunchKernelGGL(object_transform_backward_kernel, dim3((unsigned)rows), dim3(OM_THREADS), 0, (hipStream_t)stream, P, M,
                           labels, slot_of_label, R, means_out, (const float4*)rots_out, grad_means_out, (const float4*)grad_rots_out,
                           grad_means, (float4*)grad_rots, (float*)scratch);
        MGS_HIP(hipGetLastError());
    }
    if (M > 0) {
        hipLaunchKernelGGL(object_tau_final_kernel, dim3((unsigned)M), dim3(64), 0, (hipStream_t)stream, M, rows, (const float*)scratch,
                           grad_tau);
        MGS_HIP(hipGetLastError());
    }
    return 0;
}
