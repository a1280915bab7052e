// K-channel feature blending through the tables of a finished forward, and its gradient to the features.
//
// Boundary replaced: the reference blends nothing but colours; its object layer is a per-Gaussian probability row
// (gaussian_splatting/scene/gaussian_model.py:47-66 there) that the viewer turns into a per-Gaussian argmax
// (viewer/viewer_packet.py:52-54).  Here the rows are blended per pixel with the weights alpha T the colour
// forward used, so that a per-pixel object map (and a loss on it) costs one walk of the lists instead of ceil(K / 3) renders.
//
// What is read, and never written: the blend records (GeometryState::rec), the point list in blend order
// (BinningState::vals_sorted), the canonical tile ranges, n_contrib and final_T (ImageState) and the survivor masks the blend
// forward left per (64-instance step, quadrant) (BinningState::fwd_masks) -- exactly what launch_blend_backward reads, so the
// kernels are valid after an exact or a capacity-mode forward, on the global or the per-tile depth path.
//
// gfx950 mapping (tile_walk.h): a 16x16 tile is one 256-thread workgroup whose four waves never synchronise; wave w owns
// the 8x8 quadrant (w & 1, w >> 1), one pixel per lane, and walks the tile's list front to back, 64 instances per step:
//   1. the step's survivor word comes through the scalar cache (the forward is an earlier kernel), lane l loads index l;
//   2. the wave pops survivors off the word; the survivor's record (centre, conic, opacity) and its feature row arrive
//      with scalar loads off the wave-uniform index (constant address space, common.h);
//   3. all 64 lanes form alpha with tile_walk.h's falloff; a pixel takes the instance iff its list position is <= the
//      pixel's n_contrib, power <= 0 and alpha >= 1/255.  The forward decided where every pixel stops: no test of T here.
// The channels are processed in chunks of C (compile time): C accumulators per lane in the forward, C upstream gradients per
// lane in the backward; K > C walks the list ceil(K / C) times.  No LDS, no barriers.
#include "common.h"
#include "feat_walk.h"         // FeatArgs, feat_quadrant, feat_walk, make_feat_args: shared with pose_tangent.hip
#include "tile_walk.h"

#include <math.h>

namespace mgs {

namespace {

// ---- forward ---------------------------------------------------------------------------------------------------
// labels (or NULL): argmax over the K accumulated values WITHOUT the background term, ties to the lowest index, carried across
// the chunks; -1 where the forward's opacity 1 - final_T is below min_opacity.
template <int C>
__global__ void __launch_bounds__(256) features_forward_kernel(FeatArgs a, const float* __restrict__ features,
                                                               const float* __restrict__ bg, float* __restrict__ out,
                                                               int32_t* __restrict__ labels, float min_opacity) {
    const FeatQuad q = feat_quadrant(a);
    const size_t HW = (size_t)a.H * a.W;
    const float Tf = q.inside ? a.final_T[q.pix] : 1.f;
    const const_float_p feat = MGS_CONST(features), bgc = MGS_CONST(bg);
    float best = -INFINITY;
    int best_k = 0;
    for (int k0 = 0; k0 < a.K; k0 += C) {
        const int kc = min(C, a.K - k0);                  // channels of this chunk (wave-uniform)
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
        if (q.maxc != 0u)
            feat_walk(a, q, [&](uint32_t gid, float w) {
                const const_float_p f = feat + (size_t)gid * a.K + k0;     // wave-uniform: scalar loads
                if (kc == C) {
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] += f[c] * w;
                } else {                                                   // the last chunk of a K that is no multiple of C
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        if (c < kc) acc[c] += f[c] * w;
                }
            });
        if (q.inside) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (c < kc) {
                    out[(size_t)(k0 + c) * HW + q.pix] = bg ? acc[c] + Tf * bgc[k0 + c] : acc[c];
                    if (acc[c] > best) best = acc[c], best_k = k0 + c;
                }
        }
    }
    if (labels && q.inside) labels[q.pix] = (1.0f - Tf < min_opacity) ? -1 : best_k;
}

// no Gaussians: the background (or 0) and no label anywhere
__global__ void __launch_bounds__(256) features_empty_kernel(const float* __restrict__ bg, float* __restrict__ out,
                                                             int32_t* __restrict__ labels, int K, size_t HW) {
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t i = i0; i < (size_t)K * HW; i += stride) out[i] = bg ? bg[i / HW] : 0.f;
    if (labels)
        for (size_t i = i0; i < HW; i += stride) labels[i] = -1;
}

// ---- backward: packed reduction of C per-lane values over the 64 lanes -----------------------------------------------
// Each stage pairs the lanes l and l ^ d and halves the registers: the lane with bit d clear keeps the first half of the values
// and takes the partner's partial sums of them, the other lane the second half.  d = 32 and 16 are v_permlane32_swap /
// v_permlane16_swap (no select needed: the swap IS the exchange), d = 8 ... 1 go through ds_swizzle (the LDS crossbar, no
// memory).  Once one register is left the remaining stages are plain butterflies.  Value c ends up, summed over all 64 lanes,
// in the 64 / C lanes whose index is c * (64 / C) + ...: c = lane / (64 / C).
__device__ __forceinline__ float swap32_add(float x, float y) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);       // lanes 0-31: x[l] + x[l + 32]; lanes 32-63: y[l - 32] + y[l]
}
__device__ __forceinline__ float swap16_add(float x, float y) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);       // rows 0, 2: x[row] + x[row + 1]; rows 1, 3: y[row - 1] + y[row]
}
template <int XOR>
__device__ __forceinline__ float swz(float v) {                 // the value of lane l ^ XOR (XOR < 32: bit-mask mode)
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x001F | (XOR << 10)));
}
template <int M, int XOR>
__device__ __forceinline__ float reduce_in_row(const float (&c)[M], int lane) {
    if constexpr (XOR == 0) {
        static_assert(M == 1, "one register left");
        return c[0];
    } else if constexpr (M == 1) {
        const float d[1] = {c[0] + swz<XOR>(c[0])};
        return reduce_in_row<1, XOR / 2>(d, lane);
    } else {
        float d[M / 2];
        const bool hi = (lane & XOR) != 0;
#pragma unroll
        for (int i = 0; i < M / 2; ++i) {
            const float keep = hi ? c[i + M / 2] : c[i], send = hi ? c[i] : c[i + M / 2];
            d[i] = keep + swz<XOR>(send);
        }
        return reduce_in_row<M / 2, XOR / 2>(d, lane);
    }
}
template <int C>
__device__ __forceinline__ float reduce_channels(const float (&v)[C], int lane) {
    static_assert(C == 4 || C == 8 || C == 16 || C == 32, "two swap stages, then the rows");
    float b[C / 2], c[C / 4];
#pragma unroll
    for (int i = 0; i < C / 2; ++i) b[i] = swap32_add(v[i], v[i + C / 2]);       // half h holds value i + (C / 2) h
#pragma unroll
    for (int i = 0; i < C / 4; ++i) c[i] = swap16_add(b[i], b[i + C / 4]);       // row r holds value i + (C / 4) r
    return reduce_in_row<C / 4, 8>(c, lane);
}

// dL_dfeatures[g, k] += sum over the quadrant's pixels of alpha T dL_dout[k, p]: one float atomic per (instance, quadrant,
// channel), C / 16 contiguous 64-byte pieces of the Gaussian's row per instruction.  Cleared by the launcher.
template <int C>
__global__ void __launch_bounds__(256) features_backward_kernel(FeatArgs a, const float* __restrict__ dL_dout,
                                                                float* __restrict__ dL_dfeatures) {
    const FeatQuad q = feat_quadrant(a);
    if (q.maxc == 0u) return;
    const size_t HW = (size_t)a.H * a.W;
    constexpr int LPC = WAVE / C;                       // lanes that end up with the same channel's sum
    const int ch = q.lane / LPC;
    const bool writer = (q.lane % LPC) == 0;
    for (int k0 = 0; k0 < a.K; k0 += C) {
        const int kc = min(C, a.K - k0);
        float g[C];
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = (q.inside && c < kc) ? dL_dout[(size_t)(k0 + c) * HW + q.pix] : 0.f;
        float* const row0 = dL_dfeatures + k0 + ch;
        const bool store = writer && ch < kc;
        feat_walk(a, q, [&](uint32_t gid, float w) {
            float v[C];
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = w * g[c];
            const float m = reduce_channels<C>(v, q.lane);
            if (store) unsafeAtomicAdd(row0 + (size_t)gid * a.K, m);      // no-return global_atomic_add_f32
        });
    }
}

}  // namespace

// Chunk size by K: the smallest C that takes K in one walk, 16 beyond (DESIGN.md section 3 has the resource figures of each
// instantiation and why 32 is not built).
#define MGS_FEAT_DISPATCH(K_, LAUNCH) \
    do { if ((K_) <= 4) { LAUNCH(4); } else if ((K_) <= 8) { LAUNCH(8); } else { LAUNCH(16); } } while (0)

int launch_features_forward(const mgs_camera& cam, int P, int K, const GeometryState& g, const BinningState& b,
                            const ImageState& img, const float* features, const float* bg, float* out, int32_t* labels,
                            float min_opacity, hipStream_t s) {
    const int W = cam.image_width, H = cam.image_height;
    const int ntiles = tiles_x(W) * tiles_y(H);
    if (ntiles == 0) return 0;
    if (P == 0) {
        const size_t HW = (size_t)W * H, n = (size_t)K * HW;
        const size_t blocks = (n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256;
        hipLaunchKernelGGL(features_empty_kernel, dim3((unsigned)blocks), dim3(256), 0, s, bg, out, labels, K, HW);
        MGS_HIP(hipGetLastError());
        return 0;
    }
    const FeatArgs a = make_feat_args(cam, K, g, b, img);
#define FEAT_FWD(C_) hipLaunchKernelGGL(features_forward_kernel<C_>, dim3(ntiles), dim3(256), 0, s, a, features, bg, out, labels, min_opacity)
    MGS_FEAT_DISPATCH(K, FEAT_FWD);
#undef FEAT_FWD
    MGS_HIP(hipGetLastError());
    return 0;
}

int launch_features_backward(const mgs_camera& cam, int P, int K, const GeometryState& g, const BinningState& b,
                             const ImageState& img, const float* dL_dout, float* dL_dfeatures, hipStream_t s) {
    const int ntiles = tiles_x(cam.image_width) * tiles_y(cam.image_height);
    if (P == 0) return 0;
    MGS_HIP(zero_fill(dL_dfeatures, (size_t)P * K * sizeof(float), s));      // a kernel, not a memset node (common.h)
    if (ntiles == 0) return 0;
    const FeatArgs a = make_feat_args(cam, K, g, b, img);
#define FEAT_BWD(C_) hipLaunchKernelGGL(features_backward_kernel<C_>, dim3(ntiles), dim3(256), 0, s, a, dL_dout, dL_dfeatures)
    MGS_FEAT_DISPATCH(K, FEAT_BWD);
#undef FEAT_BWD
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // namespace mgs
