// Image metrics of eval_rendering() (/root/reference/utils/eval_utils.py:169-183): ONE pass over a render and its ground truth
//   c = clamp(render, 0, 1)                          -> clamped_out [3,H,W]           (:169)
//   (uint8)(c * 255.0f), channels last               -> u8_out [H,W,3], optional       (:172)
//   sum of (c - gt)^2 and the count over gt > 0, elementwise over the three planes     (:180-182)
// and a one-workgroup finalize: mse = sum / count, psnr = 20 log10(1 / sqrt(mse)) (gaussian_splatting/utils/image_utils.py:19-21).
// The SSIM of the same row is mgs_ssim_forward on clamped_out (csrc/ssim.hip), issued by the caller on the same stream.
//
// One thread takes four adjacent pixels of all three planes: three 16-byte loads per image, three 16-byte stores and the
// twelve channels-last bytes of those pixels as three 4-byte stores.  That needs every plane 16-byte aligned -- the three
// float bases 16-byte aligned, u8_out 4-byte aligned and H W a multiple of 4; anything else (an odd image, a view that starts
// inside a buffer) takes the scalar path, one pixel of three planes per thread.
//
// Sums: per-workgroup partials + a finalize that adds them in a fixed order (thread t: partials t, t + 256, ...; then the
// fixed tree of block_sum, wave_ops.h).  No atomics, no clear launch: bitwise reproducible.
// Error: the partials are carried in DOUBLE (full rate on this part, and the kernel is bound by memory).  c - gt of two floats
// is exact in double, its square and every add round at 2^-53, so sum / count carries <= (n + 2) 2^-53 relative
// (n < 2^31 terms, all of one sign: no cancellation) ~ 2.4e-7 at the very worst, 1e-10 at SLAM sizes; the stored float mse adds
// one rounding of 2^-24 = 6e-8.  The psnr is formed from the double mse, then rounded once.  The count is an exact integer
// (uint32; stored as float in the row: exact up to 2^24 elements, 5.5 megapixels).
#include "common.h"

namespace mgs {

constexpr int MT_THREADS = 256;
constexpr int MT_MAX_BLOCKS = 1024;

__device__ __forceinline__ float mt_clamp01(float r) { return r < 0.f ? 0.f : (r > 1.f ? 1.f : r); }     // (NaN stays NaN, as torch.clamp)

__device__ __forceinline__ void mt_term(float c, float g, double& acc, uint32_t& cnt) {
    const bool on = g > 0.f;
    const double d = on ? (double)c - (double)g : 0.0;
    acc = fma(d, d, acc);
    cnt += on ? 1u : 0u;
}

__device__ __forceinline__ uint32_t mt_u8(float c) { return (uint32_t)(uint8_t)(c * 255.0f); }

template <bool VEC>
__global__ void __launch_bounds__(MT_THREADS) metrics_kernel(const float* render, const float* gt, float* clamped, uint8_t* u8,
                                                             size_t HW, double* __restrict__ part_sum,
                                                             uint32_t* __restrict__ part_cnt) {
    __shared__ double s_a[4];
    __shared__ uint32_t s_n[4];
    const size_t stride = (size_t)gridDim.x * MT_THREADS;
    double acc = 0.0;
    uint32_t cnt = 0;
    if (VEC) {
        const size_t NQ = HW / 4;
        const float4 *R0 = (const float4*)render, *R1 = (const float4*)(render + HW), *R2 = (const float4*)(render + 2 * HW);
        const float4 *G0 = (const float4*)gt, *G1 = (const float4*)(gt + HW), *G2 = (const float4*)(gt + 2 * HW);
        float4 *C0 = (float4*)clamped, *C1 = (float4*)(clamped + HW), *C2 = (float4*)(clamped + 2 * HW);
        for (size_t q = (size_t)blockIdx.x * MT_THREADS + threadIdx.x; q < NQ; q += stride) {
            const float4 r0 = R0[q], r1 = R1[q], r2 = R2[q], g0 = G0[q], g1 = G1[q], g2 = G2[q];
            const float4 c0 = make_float4(mt_clamp01(r0.x), mt_clamp01(r0.y), mt_clamp01(r0.z), mt_clamp01(r0.w));
            const float4 c1 = make_float4(mt_clamp01(r1.x), mt_clamp01(r1.y), mt_clamp01(r1.z), mt_clamp01(r1.w));
            const float4 c2 = make_float4(mt_clamp01(r2.x), mt_clamp01(r2.y), mt_clamp01(r2.z), mt_clamp01(r2.w));
            C0[q] = c0; C1[q] = c1; C2[q] = c2;
            if (u8) {       // pixels 4q .. 4q + 3, channels last: bytes 12q .. 12q + 11
                uint32_t* o = (uint32_t*)(u8 + 12 * q);
                o[0] = mt_u8(c0.x) | (mt_u8(c1.x) << 8) | (mt_u8(c2.x) << 16) | (mt_u8(c0.y) << 24);
                o[1] = mt_u8(c1.y) | (mt_u8(c2.y) << 8) | (mt_u8(c0.z) << 16) | (mt_u8(c1.z) << 24);
                o[2] = mt_u8(c2.z) | (mt_u8(c0.w) << 8) | (mt_u8(c1.w) << 16) | (mt_u8(c2.w) << 24);
            }
            mt_term(c0.x, g0.x, acc, cnt); mt_term(c0.y, g0.y, acc, cnt); mt_term(c0.z, g0.z, acc, cnt); mt_term(c0.w, g0.w, acc, cnt);
            mt_term(c1.x, g1.x, acc, cnt); mt_term(c1.y, g1.y, acc, cnt); mt_term(c1.z, g1.z, acc, cnt); mt_term(c1.w, g1.w, acc, cnt);
            mt_term(c2.x, g2.x, acc, cnt); mt_term(c2.y, g2.y, acc, cnt); mt_term(c2.z, g2.z, acc, cnt); mt_term(c2.w, g2.w, acc, cnt);
        }
    } else {
        for (size_t p = (size_t)blockIdx.x * MT_THREADS + threadIdx.x; p < HW; p += stride) {
            const float r0 = render[p], r1 = render[HW + p], r2 = render[2 * HW + p];
            const float g0 = gt[p], g1 = gt[HW + p], g2 = gt[2 * HW + p];
            const float c0 = mt_clamp01(r0), c1 = mt_clamp01(r1), c2 = mt_clamp01(r2);
            clamped[p] = c0; clamped[HW + p] = c1; clamped[2 * HW + p] = c2;
            if (u8) { u8[3 * p] = (uint8_t)mt_u8(c0); u8[3 * p + 1] = (uint8_t)mt_u8(c1); u8[3 * p + 2] = (uint8_t)mt_u8(c2); }
            mt_term(c0, g0, acc, cnt); mt_term(c1, g1, acc, cnt); mt_term(c2, g2, acc, cnt);
        }
    }
    block_sum(acc, cnt, s_a, s_n);
    if (threadIdx.x == 0) { part_sum[blockIdx.x] = acc; part_cnt[blockIdx.x] = cnt; }
}

// one workgroup: row = {psnr, (ssim: not touched), mse, count}
__global__ void __launch_bounds__(MT_THREADS) metrics_finalize_kernel(const double* __restrict__ part_sum,
                                                                      const uint32_t* __restrict__ part_cnt, int nb,
                                                                      float* __restrict__ row) {
    __shared__ double s_a[4];
    __shared__ uint32_t s_n[4];
    double a = 0.0;
    uint32_t n = 0;
    for (int b = threadIdx.x; b < nb; b += MT_THREADS) { a += part_sum[b]; n += part_cnt[b]; }
    block_sum(a, n, s_a, s_n);
    if (threadIdx.x == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const double mse = n ? a / (double)n : nan;
        row[0] = (float)(n ? 20.0 * log10(1.0 / sqrt(mse)) : nan);      // mse == 0: +inf
        row[2] = (float)mse;
        row[3] = (float)n;
    }
}

static int metrics_blocks(size_t HW) {       // four pixels (twelve elements) per thread
    const size_t nb = (HW + MT_THREADS * 4 - 1) / (MT_THREADS * 4);
    return (int)(nb < 1 ? 1 : (nb > MT_MAX_BLOCKS ? MT_MAX_BLOCKS : nb));
}
static size_t metrics_cnt_offset(int nb) { return (size_t)nb * sizeof(double); }

// ---- Depth L1 between two depth images (eval_depth_l1): per-workgroup partials, one finishing workgroup -----------------------
// |a - b| of two floats is exact in double; the sums run in a fixed order (block_sum), the counts are integers.
__global__ void __launch_bounds__(MT_THREADS) depth_l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                      size_t HW, float max_depth, double* __restrict__ part_sum,
                                                                      uint32_t* __restrict__ part_cnt) {
    __shared__ double s_a[4];
    __shared__ uint32_t s_n[4], s_m[4];
    double acc = 0.0;
    uint32_t both = 0, in_b = 0;
    for (size_t p = (size_t)blockIdx.x * MT_THREADS + threadIdx.x; p < HW; p += (size_t)gridDim.x * MT_THREADS) {
        const float x = a[p], y = b[p];
        const bool on = x > 0.f && y > 0.f && (!(max_depth > 0.f) || (x <= max_depth && y <= max_depth));
        acc += on ? fabs((double)x - (double)y) : 0.0;
        both += on ? 1u : 0u;
        in_b += y > 0.f ? 1u : 0u;
    }
    block_sum(acc, both, s_a, s_n);
    in_b = block_sum(in_b, s_m);
    if (threadIdx.x == 0) { part_sum[blockIdx.x] = acc; part_cnt[2 * blockIdx.x] = both; part_cnt[2 * blockIdx.x + 1] = in_b; }
}

__global__ void __launch_bounds__(MT_THREADS) depth_l1_finish_kernel(const double* __restrict__ part_sum,
                                                                     const uint32_t* __restrict__ part_cnt, int nb,
                                                                     double* __restrict__ row) {
    __shared__ double s_a[4];
    __shared__ uint32_t s_n[4], s_m[4];
    double acc = 0.0;
    uint32_t both = 0, in_b = 0;                 // (an image holds at most 2^28 pixels)
    for (int i = threadIdx.x; i < nb; i += MT_THREADS) { acc += part_sum[i]; both += part_cnt[2 * i]; in_b += part_cnt[2 * i + 1]; }
    block_sum(acc, both, s_a, s_n);
    in_b = block_sum(in_b, s_m);
    if (threadIdx.x == 0) { row[0] = acc; row[1] = (double)both; row[2] = (double)in_b; }
}
static int depth_l1_blocks(size_t HW) {
    const size_t nb = (HW + MT_THREADS * 4 - 1) / (MT_THREADS * 4);
    return (int)(nb < 1 ? 1 : (nb > MT_MAX_BLOCKS ? MT_MAX_BLOCKS : nb));
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_metrics_scratch_bytes(int32_t width, int32_t height) {
    const int nb = (width < 1 || height < 1) ? 1 : metrics_blocks((size_t)width * height);
    return (metrics_cnt_offset(nb) + (size_t)nb * sizeof(uint32_t) + 15) & ~(size_t)15;
}

int mgs_image_metrics(int32_t width, int32_t height, const float* render, const float* gt, float* clamped_out, uint8_t* u8_out,
                      void* scratch, float* row_out, void* stream) {
    if (width < 1 || height < 1) { set_error("image size must be positive"); return 1; }
    if (3 * (size_t)width * height >= ((size_t)1 << 31)) { set_error("3 x width x height must stay below 2^31"); return 1; }
    if (!render || !gt || !clamped_out || !scratch || !row_out) {
        set_error("render, gt, clamped_out, scratch and row_out must be non-NULL");
        return 1;
    }
    if ((size_t)scratch % 8) { set_error("scratch must be 8-byte aligned"); return 1; }
    const size_t HW = (size_t)width * height;
    const int nb = metrics_blocks(HW);
    double* part_sum = (double*)scratch;
    uint32_t* part_cnt = (uint32_t*)((char*)scratch + metrics_cnt_offset(nb));
    hipStream_t s = (hipStream_t)stream;
    auto al = [](const void* p, size_t n) { return ((size_t)p % n) == 0; };
    if (HW % 4 == 0 && al(render, 16) && al(gt, 16) && al(clamped_out, 16) && al(u8_out, 4))
        hipLaunchKernelGGL(metrics_kernel<true>, dim3(nb), dim3(MT_THREADS), 0, s, render, gt, clamped_out, u8_out, HW, part_sum, part_cnt);
    else
        hipLaunchKernelGGL(metrics_kernel<false>, dim3(nb), dim3(MT_THREADS), 0, s, render, gt, clamped_out, u8_out, HW, part_sum, part_cnt);
    hipLaunchKernelGGL(metrics_finalize_kernel, dim3(1), dim3(MT_THREADS), 0, s, part_sum, part_cnt, nb, row_out);
    MGS_HIP(hipGetLastError());
    return 0;
}

size_t mgs_depth_l1_scratch_bytes(void) { return (size_t)MT_MAX_BLOCKS * (sizeof(double) + 2 * sizeof(uint32_t)) + 256; }

int mgs_depth_l1(int32_t W, int32_t H, const float* a, const float* b, float max_depth, double* row, void* scratch, void* stream) {
    const char* who = "mgs_depth_l1";
    if (W < 1 || H < 1 || W > MGS_MESH_RENDER_MAX_IMAGE || H > MGS_MESH_RENDER_MAX_IMAGE) {
        set_error("%s: the image must be 1 .. %d pixels wide and high", who, MGS_MESH_RENDER_MAX_IMAGE);
        return 1;
    }
    if (!a || !b || !row || !scratch) { set_error("%s: a, b, row and scratch must be non-NULL", who); return 1; }
    const size_t HW = (size_t)W * H;
    const int nb = depth_l1_blocks(HW);
    ScratchCursor c(scratch);
    double* part_sum = c.take<double>((size_t)MT_MAX_BLOCKS * sizeof(double));
    uint32_t* part_cnt = c.take<uint32_t>((size_t)MT_MAX_BLOCKS * 2 * sizeof(uint32_t));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_l1_partial_kernel, dim3(nb), dim3(MT_THREADS), 0, s, a, b, HW, max_depth, part_sum, part_cnt);
    hipLaunchKernelGGL(depth_l1_finish_kernel, dim3(1), dim3(MT_THREADS), 0, s, part_sum, part_cnt, nb, row);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
