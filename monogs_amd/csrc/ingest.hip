// Frame ingest: what MonocularDataset.__getitem__ (/root/reference/utils/dataset.py:410-508) and
// CameraExtrinsics.compute_grad_mask (/root/reference/utils/camera_utils.py:184-212, utils/slam_utils.py:6-40) do to a decoded
// frame, on the device:
//   prepare    8-bit colour [H][W][3] (optionally resampled through an undistortion map, the integer bilinear scheme of an
//              8-bit INTER_LINEAR remap with a constant-zero border) -> float [3][H][W] = float32(double(v) / 255.0)   (:452-465)
//              16-bit depth -> float32(double(v) / depth_scale)                                                         (:431,468)
//              segmentation ids + a 256-bit set of masked ids -> 0/1 mask                                               (:445-449)
//   intensity  grey = (r + g + b) / 3, Scharr gradients of the reflect-padded grey image normalised by 1/32, zeroed where a
//              3x3 neighbourhood holds |grey| <= eps, intensity = sqrt(gv^2 + gh^2)            (slam_utils.py:6-40, :187-192)
//   median     the lower median of the H W intensities: mgs_masked_median (csrc/kfwindow.hip), lo = -inf, no mask      (:211)
//   threshold  grad_mask = intensity > __fmul_rn(median, edge_threshold)                                                (:212)
// One + one + six + one launches, stream-ordered, nothing assumed of scratch or outputs on entry, no atomics, no LDS.
//
// Every kernel has a route that moves 16 bytes per access (four adjacent pixels per thread: needs every base 16-byte aligned
// and W a multiple of 4, so that a group of four never straddles two rows) and a scalar route, one pixel per thread, for
// anything else.  The remap's four source taps are gathers on either route; only its maps and outputs are vectorised.
//
// Out-of-range maps: the fixed-point coordinate is tested as a FLOAT before it is converted (NaN fails the test), a source tap
// is read only when 0 <= x < W and 0 <= y < H: no map value whatsoever reads outside the source image.
#include <math.h>

#include "common.h"

namespace mgs {

constexpr int IG_THREADS = 256;

struct IngestArgs {
    const uint8_t* rgb_u8;
    const float* map_x;
    const float* map_y;
    const uint16_t* depth_u16;
    const uint8_t* segmentation;
    float* rgb_out;
    float* depth_out;
    uint8_t* mask_out;
    double depth_scale;
    uint32_t ids[8];
    int W, H;
};

__device__ __forceinline__ float ig_colour(uint32_t v) { return (float)((double)v / 255.0); }

// bit `id` of the 256-bit set: a select chain over the eight words (an indexed read of a kernel argument would go through
// scratch memory)
__device__ __forceinline__ uint32_t ig_masked(const IngestArgs& a, uint32_t id) {
    const uint32_t k = id >> 5;
    const uint32_t lo = k & 2 ? (k & 1 ? a.ids[3] : a.ids[2]) : (k & 1 ? a.ids[1] : a.ids[0]);
    const uint32_t hi = k & 2 ? (k & 1 ? a.ids[7] : a.ids[6]) : (k & 1 ? a.ids[5] : a.ids[4]);
    return ((k & 4 ? hi : lo) >> (id & 31)) & 1u;
}

// one pixel of the 8-bit remap: fixed-point coordinates with 5 fractional bits, integer weights that sum to 2^15
__device__ __forceinline__ void ig_remap(const uint8_t* __restrict__ src, int W, int H, float mx, float my, uint32_t& r,
                                         uint32_t& g, uint32_t& b) {
    const float fx = rintf(mx * 32.0f), fy = rintf(my * 32.0f);          // round half to even; NaN stays NaN
    r = g = b = 0;
    if (!(fx >= -32.0f && fx < 32.0f * (float)W && fy >= -32.0f && fy < 32.0f * (float)H)) return;   // every tap outside
    const int sx = (int)fx, sy = (int)fy;
    const int ix = sx >> 5, iy = sy >> 5;                                 // arithmetic shifts: -1 for sx in [-32, -1]
    const uint32_t ax = (uint32_t)(sx & 31), ay = (uint32_t)(sy & 31);
    const bool x0 = ix >= 0, x1 = ix + 1 < W, y0 = iy >= 0, y1 = iy + 1 < H;   // (ix <= W - 1 and iy <= H - 1 hold here)
    const uint32_t w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
    uint32_t sr = 16384, sg = 16384, sb = 16384;
    if (y0 && x0) { const uint8_t* p = src + 3 * ((size_t)iy * W + ix);           sr += w00 * p[0]; sg += w00 * p[1]; sb += w00 * p[2]; }
    if (y0 && x1) { const uint8_t* p = src + 3 * ((size_t)iy * W + ix + 1);       sr += w01 * p[0]; sg += w01 * p[1]; sb += w01 * p[2]; }
    if (y1 && x0) { const uint8_t* p = src + 3 * ((size_t)(iy + 1) * W + ix);     sr += w10 * p[0]; sg += w10 * p[1]; sb += w10 * p[2]; }
    if (y1 && x1) { const uint8_t* p = src + 3 * ((size_t)(iy + 1) * W + ix + 1); sr += w11 * p[0]; sg += w11 * p[1]; sb += w11 * p[2]; }
    r = sr >> 15; g = sg >> 15; b = sb >> 15;
}

template <bool VEC, bool REMAP>
__global__ void __launch_bounds__(IG_THREADS) ingest_prepare_kernel(const IngestArgs a) {
    const size_t HW = (size_t)a.W * a.H;
    const size_t t = (size_t)blockIdx.x * IG_THREADS + threadIdx.x;
    if (VEC) {
        if (t >= HW / 4) return;
        uint32_t c[12];                                                   // pixels 4t .. 4t + 3, channels last
        if (REMAP) {
            const float4 mx = ((const float4*)a.map_x)[t], my = ((const float4*)a.map_y)[t];
            ig_remap(a.rgb_u8, a.W, a.H, mx.x, my.x, c[0], c[1], c[2]);
            ig_remap(a.rgb_u8, a.W, a.H, mx.y, my.y, c[3], c[4], c[5]);
            ig_remap(a.rgb_u8, a.W, a.H, mx.z, my.z, c[6], c[7], c[8]);
            ig_remap(a.rgb_u8, a.W, a.H, mx.w, my.w, c[9], c[10], c[11]);
        } else {
            const uint32_t* p = (const uint32_t*)(a.rgb_u8 + 12 * t);
            const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
            c[0] = w0 & 255; c[1] = (w0 >> 8) & 255; c[2] = (w0 >> 16) & 255; c[3] = w0 >> 24;
            c[4] = w1 & 255; c[5] = (w1 >> 8) & 255; c[6] = (w1 >> 16) & 255; c[7] = w1 >> 24;
            c[8] = w2 & 255; c[9] = (w2 >> 8) & 255; c[10] = (w2 >> 16) & 255; c[11] = w2 >> 24;
        }
        ((float4*)a.rgb_out)[t] = make_float4(ig_colour(c[0]), ig_colour(c[3]), ig_colour(c[6]), ig_colour(c[9]));
        ((float4*)(a.rgb_out + HW))[t] = make_float4(ig_colour(c[1]), ig_colour(c[4]), ig_colour(c[7]), ig_colour(c[10]));
        ((float4*)(a.rgb_out + 2 * HW))[t] = make_float4(ig_colour(c[2]), ig_colour(c[5]), ig_colour(c[8]), ig_colour(c[11]));
        if (a.depth_u16) {
            const uint2 d = ((const uint2*)a.depth_u16)[t];
            ((float4*)a.depth_out)[t] = make_float4((float)((double)(d.x & 0xffffu) / a.depth_scale), (float)((double)(d.x >> 16) / a.depth_scale),
                                                    (float)((double)(d.y & 0xffffu) / a.depth_scale), (float)((double)(d.y >> 16) / a.depth_scale));
        }
        uint32_t m = 0x01010101u;
        if (a.segmentation) {
            const uint32_t s = ((const uint32_t*)a.segmentation)[t];
            m ^= ig_masked(a, s & 255) | (ig_masked(a, (s >> 8) & 255) << 8) | (ig_masked(a, (s >> 16) & 255) << 16) | (ig_masked(a, s >> 24) << 24);
        }
        ((uint32_t*)a.mask_out)[t] = m;
    } else {
        if (t >= HW) return;
        uint32_t r, g, b;
        if (REMAP) ig_remap(a.rgb_u8, a.W, a.H, a.map_x[t], a.map_y[t], r, g, b);
        else { r = a.rgb_u8[3 * t]; g = a.rgb_u8[3 * t + 1]; b = a.rgb_u8[3 * t + 2]; }
        a.rgb_out[t] = ig_colour(r); a.rgb_out[HW + t] = ig_colour(g); a.rgb_out[2 * HW + t] = ig_colour(b);
        if (a.depth_u16) a.depth_out[t] = (float)((double)a.depth_u16[t] / a.depth_scale);
        a.mask_out[t] = (uint8_t)(a.segmentation ? 1u ^ ig_masked(a, a.segmentation[t]) : 1u);
    }
}

__device__ __forceinline__ float ig_gray(float r, float g, float b) { return (r + g + b) / 3.0f; }

// gradient intensity of the centre of a 3x3 grey neighbourhood (rows top, mid, bottom; columns 0..2)
__device__ __forceinline__ float ig_intensity(float t0, float t1, float t2, float m0, float m1, float m2, float b0, float b1,
                                              float b2, float eps) {
    const bool valid = fabsf(t0) > eps && fabsf(t1) > eps && fabsf(t2) > eps && fabsf(m0) > eps && fabsf(m1) > eps &&
                       fabsf(m2) > eps && fabsf(b0) > eps && fabsf(b1) > eps && fabsf(b2) > eps;
    const float gv = ((3.0f * t0 + 10.0f * t1 + 3.0f * t2) - (3.0f * b0 + 10.0f * b1 + 3.0f * b2)) * 0.03125f;
    const float gh = ((3.0f * t0 + 10.0f * m0 + 3.0f * b0) - (3.0f * t2 + 10.0f * m2 + 3.0f * b2)) * 0.03125f;
    return valid ? sqrtf(gv * gv + gh * gh) : 0.0f;
}

template <bool VEC>
__global__ void __launch_bounds__(IG_THREADS) ingest_intensity_kernel(const float* __restrict__ rgb, int W, int H, float eps,
                                                                      float* __restrict__ intensity) {
    const size_t HW = (size_t)W * H;
    const size_t t = (size_t)blockIdx.x * IG_THREADS + threadIdx.x;
    const float *R = rgb, *G = rgb + HW, *B = rgb + 2 * HW;
    if (VEC) {
        if (t >= HW / 4) return;
        const int Wq = W / 4;
        const int y = (int)(t / Wq), x = 4 * (int)(t % Wq);
        const int rows[3] = {y == 0 ? 1 : y - 1, y, y == H - 1 ? H - 2 : y + 1};       // reflect padding: -1 -> 1, H -> H - 2
        const int xl = x == 0 ? 1 : x - 1, xr = x + 4 == W ? W - 2 : x + 4;
        float g[3][6];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t o = (size_t)rows[k] * W;
            const float4 r4 = *(const float4*)(R + o + x), g4 = *(const float4*)(G + o + x), b4 = *(const float4*)(B + o + x);
            g[k][0] = ig_gray(R[o + xl], G[o + xl], B[o + xl]);
            g[k][1] = ig_gray(r4.x, g4.x, b4.x); g[k][2] = ig_gray(r4.y, g4.y, b4.y);
            g[k][3] = ig_gray(r4.z, g4.z, b4.z); g[k][4] = ig_gray(r4.w, g4.w, b4.w);
            g[k][5] = ig_gray(R[o + xr], G[o + xr], B[o + xr]);
        }
        float o4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o4[j] = ig_intensity(g[0][j], g[0][j + 1], g[0][j + 2], g[1][j], g[1][j + 1], g[1][j + 2], g[2][j], g[2][j + 1],
                                 g[2][j + 2], eps);
        ((float4*)intensity)[t] = make_float4(o4[0], o4[1], o4[2], o4[3]);
    } else {
        if (t >= HW) return;
        const int y = (int)(t / W), x = (int)(t % W);
        const int rows[3] = {y == 0 ? 1 : y - 1, y, y == H - 1 ? H - 2 : y + 1};
        const int cols[3] = {x == 0 ? 1 : x - 1, x, x == W - 1 ? W - 2 : x + 1};
        float g[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const size_t o = (size_t)rows[k] * W + cols[j];
                g[k][j] = ig_gray(R[o], G[o], B[o]);
            }
        intensity[t] = ig_intensity(g[0][0], g[0][1], g[0][2], g[1][0], g[1][1], g[1][2], g[2][0], g[2][1], g[2][2], eps);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(IG_THREADS) ingest_threshold_kernel(const float* __restrict__ intensity,
                                                                      const float* __restrict__ median, float edge_threshold,
                                                                      size_t HW, uint8_t* __restrict__ grad_mask) {
    const size_t t = (size_t)blockIdx.x * IG_THREADS + threadIdx.x;
    const float thr = __fmul_rn(median[0], edge_threshold);
    if (VEC) {
        if (t >= HW / 4) return;
        const float4 v = ((const float4*)intensity)[t];
        ((uint32_t*)grad_mask)[t] = (v.x > thr ? 1u : 0u) | (v.y > thr ? 0x100u : 0u) | (v.z > thr ? 0x10000u : 0u) |
                                    (v.w > thr ? 0x1000000u : 0u);
    } else {
        if (t >= HW) return;
        grad_mask[t] = intensity[t] > thr ? 1 : 0;
    }
}

// scratch: 16 bytes {median, count, -, -}, the intensity image (used when the caller wants none), the median's scratch
constexpr size_t IG_HDR = 16;
static size_t ig_intensity_bytes(size_t HW) { return align_up(HW * sizeof(float), 16); }
static unsigned ig_blocks(size_t items) { return (unsigned)((items + IG_THREADS - 1) / IG_THREADS); }
static bool ig_al16(const void* p) { return ((size_t)p % 16) == 0; }

static const char* ig_size_error(int32_t width, int32_t height) {
    if (width < 2 || height < 2) return "width and height must be at least 2 (reflect padding)";
    if (3 * (size_t)width * height >= ((size_t)1 << 31)) return "3 x width x height must stay below 2^31";
    return nullptr;
}

// the intensity, median and threshold launches; every argument has been checked
static int ig_grad_mask_launch(int W, int H, const float* rgb, float edge_threshold, float eps, void* scratch,
                               uint8_t* grad_mask_out, float* intensity_out, hipStream_t s) {
    const size_t HW = (size_t)W * H;
    float* median = (float*)scratch;
    uint32_t* count = (uint32_t*)scratch + 1;
    float* intensity = intensity_out ? intensity_out : (float*)((char*)scratch + IG_HDR);
    void* median_scratch = (char*)scratch + IG_HDR + ig_intensity_bytes(HW);
    const bool vec = W % 4 == 0 && ig_al16(rgb) && ig_al16(intensity) && ig_al16(grad_mask_out);
    if (vec) hipLaunchKernelGGL(ingest_intensity_kernel<true>, dim3(ig_blocks(HW / 4)), dim3(IG_THREADS), 0, s, rgb, W, H, eps, intensity);
    else hipLaunchKernelGGL(ingest_intensity_kernel<false>, dim3(ig_blocks(HW)), dim3(IG_THREADS), 0, s, rgb, W, H, eps, intensity);
    const int rc = mgs_masked_median(intensity, nullptr, HW, -INFINITY, median_scratch, median, count, s);
    if (rc != 0) return rc;
    if (vec) hipLaunchKernelGGL(ingest_threshold_kernel<true>, dim3(ig_blocks(HW / 4)), dim3(IG_THREADS), 0, s, intensity, median, edge_threshold, HW, grad_mask_out);
    else hipLaunchKernelGGL(ingest_threshold_kernel<false>, dim3(ig_blocks(HW)), dim3(IG_THREADS), 0, s, intensity, median, edge_threshold, HW, grad_mask_out);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_grad_mask_scratch_bytes(int32_t width, int32_t height) {
    const size_t HW = (width < 1 || height < 1) ? 1 : (size_t)width * height;
    return IG_HDR + ig_intensity_bytes(HW) + align_up(mgs_median_scratch_bytes(HW), 16);
}

int mgs_grad_mask(int32_t width, int32_t height, const float* rgb, float edge_threshold, float eps, void* scratch,
                  uint8_t* grad_mask_out, float* intensity_out, void* stream) {
    if (const char* e = ig_size_error(width, height)) { set_error("mgs_grad_mask: %s", e); return 1; }
    if (!rgb || !scratch || !grad_mask_out) { set_error("mgs_grad_mask: rgb, scratch and grad_mask_out must be non-NULL"); return 1; }
    if (!ig_al16(scratch)) { set_error("mgs_grad_mask: scratch must be 16-byte aligned"); return 1; }
    return ig_grad_mask_launch(width, height, rgb, edge_threshold, eps, scratch, grad_mask_out, intensity_out, (hipStream_t)stream);
}

int mgs_frame_prepare(const MgsFramePrepare* p, void* stream) {
    if (!p) { set_error("mgs_frame_prepare: params must be non-NULL"); return 1; }
    if (const char* e = ig_size_error(p->width, p->height)) { set_error("mgs_frame_prepare: %s", e); return 1; }
    if (!p->rgb_u8 || !p->rgb_out || !p->mask_out || !p->grad_mask_out || !p->scratch) {
        set_error("mgs_frame_prepare: rgb_u8, rgb_out, mask_out, grad_mask_out and scratch must be non-NULL");
        return 1;
    }
    if (!ig_al16(p->scratch)) { set_error("mgs_frame_prepare: scratch must be 16-byte aligned"); return 1; }
    if ((p->map_x == nullptr) != (p->map_y == nullptr)) { set_error("mgs_frame_prepare: map_x and map_y go together: both or neither"); return 1; }
    if ((p->depth_u16 == nullptr) != (p->depth_out == nullptr)) {
        set_error("mgs_frame_prepare: depth_u16 and depth_out go together: both or neither");
        return 1;
    }
    if (p->depth_u16 && !(p->depth_scale > 0.0 && p->depth_scale < (double)INFINITY)) {
        set_error("mgs_frame_prepare: depth_scale must be positive and finite");
        return 1;
    }
    IngestArgs a;
    a.rgb_u8 = p->rgb_u8; a.map_x = p->map_x; a.map_y = p->map_y; a.depth_u16 = p->depth_u16; a.segmentation = p->segmentation;
    a.rgb_out = p->rgb_out; a.depth_out = p->depth_out; a.mask_out = p->mask_out;
    a.depth_scale = p->depth_u16 ? p->depth_scale : 1.0;
    for (int i = 0; i < 8; ++i) a.ids[i] = p->masked_ids[i];
    a.W = p->width; a.H = p->height;
    const size_t HW = (size_t)a.W * a.H;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = a.W % 4 == 0 && ig_al16(a.rgb_u8) && ig_al16(a.map_x) && ig_al16(a.map_y) && ig_al16(a.depth_u16) &&
                     ig_al16(a.segmentation) && ig_al16(a.rgb_out) && ig_al16(a.depth_out) && ig_al16(a.mask_out);
    const bool remap = a.map_x != nullptr;
    const dim3 grid(ig_blocks(vec ? HW / 4 : HW)), block(IG_THREADS);
    if (vec && remap) hipLaunchKernelGGL((ingest_prepare_kernel<true, true>), grid, block, 0, s, a);
    else if (vec) hipLaunchKernelGGL((ingest_prepare_kernel<true, false>), grid, block, 0, s, a);
    else if (remap) hipLaunchKernelGGL((ingest_prepare_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ingest_prepare_kernel<false, false>), grid, block, 0, s, a);
    return ig_grad_mask_launch(a.W, a.H, a.rgb_out, p->edge_threshold, p->eps, p->scratch, p->grad_mask_out, p->intensity_out, s);
}

}  // extern "C"
