// The object layer's loss and its score: softmax cross-entropy of a blended K-channel image against 8-bit ids, value +
// gradient to the image, and the confusion matrix of rendered labels against ground-truth ids.
//
// Boundary replaced: the reference never learns its object rows ("set requires grad to True" is a TODO at
// gaussian_splatting/scene/gaussian_model.py:381) and measures no label accuracy.  Here the image mgs_features_forward blends
// from the RAW rows is taken as logits; d_feat is what mgs_features_backward turns into the gradient of the rows.
//
//   counted(p) = (valid == NULL || valid[p] != 0) && labels[p] < K,  N = number of counted pixels
//   L          = (1 / N) sum_counted [ logsumexp_k feat[k, p] - feat[labels[p], p] ]
//   d_feat[k, p] = (softmax_k(feat[:, p]) - [k == labels[p]]) / N on counted pixels, exactly 0 elsewhere;  N == 0: L = 0, d_feat = 0
//
// prepare (once per keyframe: N depends on labels and valid alone): per-workgroup integer partials + a one-workgroup finalize.
// loss + gradients (per iteration, two launches): label_loss_kernel reads feat, writes d_feat and one partial sum per
// workgroup; label_finalize_kernel adds the partials in a fixed order.  No atomics, no clear launch, nothing assumed of scratch
// or outputs on entry, no host synchronisation: loss and gradient are bitwise reproducible.
//
// A lane owns four adjacent pixels (16-byte loads and stores of every channel plane; needs W % 4 == 0 and every base 16-byte
// aligned, as ingest.hip) or one pixel (anything else).  Per pixel: m = max_k x_k, s = sum_k exp(x_k - m) carried in DOUBLE --
// a float sum next to a term of 1 loses the small terms that decide softmax - 1 at a confident label -- then
//   loss term  (m - x_label) + log(s)                       (the first difference is exact wherever the label is the maximum)
//   gradient   exp(x_k - m) * (1 / (s N)),  at the label (exp(x_label - m) - s) / (s N) formed in double
// K <= KC (compile time: 8, 24): the pixel's K values stay in registers, feat is read once and exp is taken once per value.
// Beyond: an online max / sum pass (one exp per value) and a second read of feat (out of L2: a lane re-reads its own
// addresses) for the gradient.  Sums over pixels: double, per-lane, then a fixed tree (metrics.hip has the error argument).
//
// confusion: counts[gt, pred] += 1 over the counted pixels whose prediction lies in 0 .. K-1, side[0] += the counted pixels
// without one (-1 = not seen), side[1] += the pixels not counted.  Integer atomics only (exact, order-free): a workgroup stages
// its K x K counts in LDS while they fit in 16 KiB (K <= 64) and flushes the non-zero ones; beyond, global atomics per pixel.
#include "common.h"

#include <math.h>

namespace mgs {

constexpr int LB_THREADS = 256;
constexpr int LB_MAX_BLOCKS = 2048;
constexpr size_t LB_PART = 16;           // scratch: [0] float loss, [1..3] unused, then one 8-byte partial per workgroup
constexpr int LB_LDS_K = 64;             // K x K x 4 bytes <= 16 KiB
constexpr int LB_BATCH = 8;              // channels whose loads are in flight together on the two-pass route

struct LabelArgs {
    const float* feat;
    const uint8_t* labels;
    const uint8_t* valid;
    const uint32_t* count;               // {N, pixels not counted} as mgs_label_prepare left them
    float* d_feat;
    int W, H, K;
};

static bool lb_al(const void* p, size_t n) { return ((size_t)p % n) == 0; }
static int lb_blocks(size_t items) {
    const size_t nb = (items + LB_THREADS - 1) / LB_THREADS;
    return (int)(nb < 1 ? 1 : (nb > LB_MAX_BLOCKS ? LB_MAX_BLOCKS : nb));
}

// the ids and the counted flags of the lane's PIX pixels (group q)
template <int PIX>
__device__ __forceinline__ void lb_ids(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ valid, int K, size_t q,
                                       uint32_t (&lab)[PIX], bool (&on)[PIX]) {
    if (PIX == 4) {
        const uint32_t l = ((const uint32_t*)labels)[q], v = valid ? ((const uint32_t*)valid)[q] : 0x01010101u;
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            lab[j] = (l >> (8 * j)) & 255u;
            on[j] = ((v >> (8 * j)) & 255u) != 0u && lab[j] < (uint32_t)K;
        }
    } else {
        lab[0] = labels[q];
        on[0] = (valid ? valid[q] != 0 : true) && lab[0] < (uint32_t)K;
    }
}

template <int PIX>
__device__ __forceinline__ void lb_load(const float* __restrict__ plane, size_t q, float (&x)[PIX]) {
    if (PIX == 4) {
        const float4 v = ((const float4*)plane)[q];
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
        x[0] = plane[q];
    }
}
template <int PIX>
__device__ __forceinline__ void lb_store(float* __restrict__ plane, size_t q, const float (&g)[PIX]) {
    if (PIX == 4) ((float4*)plane)[q] = make_float4(g[0], g[1], g[2], g[3]);
    else plane[q] = g[0];
}

// ---- prepare: N ------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(LB_THREADS) label_count_kernel(const uint8_t* __restrict__ labels,
                                                                 const uint8_t* __restrict__ valid, int K, size_t HW,
                                                                 uint32_t* __restrict__ part) {
    constexpr int PIX = VEC ? 4 : 1;
    __shared__ uint32_t s_n[4];
    const size_t NG = HW / PIX, stride = (size_t)gridDim.x * LB_THREADS;
    uint32_t n = 0;
    for (size_t q = (size_t)blockIdx.x * LB_THREADS + threadIdx.x; q < NG; q += stride) {
        uint32_t lab[PIX];
        bool on[PIX];
        lb_ids<PIX>(labels, valid, K, q, lab, on);
#pragma unroll
        for (int j = 0; j < PIX; ++j) n += on[j] ? 1u : 0u;
    }
    n = block_sum(n, s_n);
    if (threadIdx.x == 0) part[blockIdx.x] = n;
}

__global__ void __launch_bounds__(LB_THREADS) label_count_finalize_kernel(const uint32_t* __restrict__ part, int nb, uint32_t HW,
                                                                          uint32_t* __restrict__ count_out) {
    __shared__ uint32_t s_n[4];
    uint32_t n = 0;
    for (int b = threadIdx.x; b < nb; b += LB_THREADS) n += part[b];
    n = block_sum(n, s_n);
    if (threadIdx.x == 0) { count_out[0] = n; count_out[1] = HW - n; }
}

// ---- loss + gradient -------------------------------------------------------------------------------------------------
// what a pixel keeps between the two passes
template <int PIX>
struct LbPixel {
    float m[PIX];             // max_k x_k
    float c[PIX];             // 1 / (s N), 0 where the pixel is not counted
    float gl[PIX];            // the gradient at the label
};

// from m, s and x_label: the loss term (returned), c and gl
template <int PIX>
__device__ __forceinline__ double lb_finish(const float (&m)[PIX], const double (&s)[PIX], const float (&xl)[PIX],
                                            const bool (&on)[PIX], double inv_n, LbPixel<PIX>& px) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const double c = inv_n / s[j];                           // s >= 1: the maximum contributes exp(0)
        const double el = (double)expf(xl[j] - m[j]);
        px.m[j] = m[j];
        px.c[j] = on[j] ? (float)c : 0.f;
        px.gl[j] = on[j] ? (float)((el - s[j]) * c) : 0.f;
        acc += on[j] ? (double)((m[j] - xl[j]) + logf((float)s[j])) : 0.0;
    }
    return acc;
}

template <bool VEC, int KC>
__global__ void __launch_bounds__(LB_THREADS) label_loss_kernel(const LabelArgs a, double* __restrict__ part) {
    constexpr int PIX = VEC ? 4 : 1;
    __shared__ double s_a[4];
    const size_t HW = (size_t)a.W * a.H, NG = HW / PIX, stride = (size_t)gridDim.x * LB_THREADS;
    const uint32_t n = a.count[0];
    const double inv_n = n ? 1.0 / (double)n : 0.0;
    const int K = a.K;
    double acc = 0.0;
    for (size_t q = (size_t)blockIdx.x * LB_THREADS + threadIdx.x; q < NG; q += stride) {
        uint32_t lab[PIX];
        bool on[PIX];
        lb_ids<PIX>(a.labels, a.valid, K, q, lab, on);
        float m[PIX], xl[PIX];
        double s[PIX];
        LbPixel<PIX> px;
#pragma unroll
        for (int j = 0; j < PIX; ++j) m[j] = -INFINITY, xl[j] = 0.f, s[j] = 0.0;
        if (KC > 0) {
            // K <= KC values per pixel in registers: max, then exp once per value (kept in place of the value), then the products
            float x[KC > 0 ? KC : 1][PIX];
#pragma unroll
            for (int k = 0; k < KC; ++k)
                if (k < K) lb_load<PIX>(a.feat + (size_t)k * HW, q, x[k]);
#pragma unroll
            for (int k = 0; k < KC; ++k)
                if (k < K) {
#pragma unroll
                    for (int j = 0; j < PIX; ++j) {
                        m[j] = fmaxf(m[j], x[k][j]);
                        xl[j] = (uint32_t)k == lab[j] ? x[k][j] : xl[j];
                    }
                }
#pragma unroll
            for (int k = 0; k < KC; ++k)
                if (k < K) {
#pragma unroll
                    for (int j = 0; j < PIX; ++j) {
                        x[k][j] = expf(x[k][j] - m[j]);
                        s[j] += (double)x[k][j];
                    }
                }
            acc += lb_finish<PIX>(m, s, xl, on, inv_n, px);
#pragma unroll
            for (int k = 0; k < KC; ++k)
                if (k < K) {
                    float g[PIX];
#pragma unroll
                    for (int j = 0; j < PIX; ++j) g[j] = (uint32_t)k == lab[j] ? px.gl[j] : x[k][j] * px.c[j];
                    lb_store<PIX>(a.d_feat + (size_t)k * HW, q, g);
                }
        } else {
            // online: one exp per value, whichever of the running maximum and the value is the larger.  The channels come in
            // batches of LB_BATCH whose loads are all issued before the first is used: a lane that waits for one 16-byte load
            // per channel is bound by the latency of K dependent round trips, not by bytes.
            for (int k0 = 0; k0 < K; k0 += LB_BATCH) {
                float x[LB_BATCH][PIX];
#pragma unroll
                for (int c = 0; c < LB_BATCH; ++c)
                    if (k0 + c < K) lb_load<PIX>(a.feat + (size_t)(k0 + c) * HW, q, x[c]);
#pragma unroll
                for (int c = 0; c < LB_BATCH; ++c)
                    if (k0 + c < K) {
#pragma unroll
                        for (int j = 0; j < PIX; ++j) {
                            const float d = x[c][j] - m[j];               // +inf at k = 0: e = 0, s = 0 * 0 + 1
                            const double e = (double)expf(-fabsf(d));
                            s[j] = d > 0.f ? fma(s[j], e, 1.0) : s[j] + e;
                            m[j] = d > 0.f ? x[c][j] : m[j];
                            xl[j] = (uint32_t)(k0 + c) == lab[j] ? x[c][j] : xl[j];
                        }
                    }
            }
            acc += lb_finish<PIX>(m, s, xl, on, inv_n, px);
            for (int k0 = 0; k0 < K; k0 += LB_BATCH) {
                float x[LB_BATCH][PIX];
#pragma unroll
                for (int c = 0; c < LB_BATCH; ++c)
                    if (k0 + c < K) lb_load<PIX>(a.feat + (size_t)(k0 + c) * HW, q, x[c]);
#pragma unroll
                for (int c = 0; c < LB_BATCH; ++c)
                    if (k0 + c < K) {
                        float g[PIX];
#pragma unroll
                        for (int j = 0; j < PIX; ++j)
                            g[j] = (uint32_t)(k0 + c) == lab[j] ? px.gl[j] : expf(x[c][j] - px.m[j]) * px.c[j];
                        lb_store<PIX>(a.d_feat + (size_t)(k0 + c) * HW, q, g);
                    }
            }
        }
    }
    acc = block_sum(acc, s_a);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(LB_THREADS) label_finalize_kernel(const double* __restrict__ part, int nb,
                                                                    const uint32_t* __restrict__ count, float* __restrict__ loss) {
    __shared__ double s_a[4];
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += LB_THREADS) a += part[b];
    a = block_sum(a, s_a);
    if (threadIdx.x == 0) loss[0] = count[0] ? (float)(a / (double)count[0]) : 0.f;
}

// ---- confusion -------------------------------------------------------------------------------------------------------
template <bool LDS>
__global__ void __launch_bounds__(LB_THREADS) label_confusion_kernel(const int32_t* __restrict__ pred,
                                                                     const uint8_t* __restrict__ gt,
                                                                     const uint8_t* __restrict__ valid, int K, size_t HW,
                                                                     uint32_t* __restrict__ counts, uint32_t* __restrict__ side) {
    __shared__ uint32_t s_c[LDS ? LB_LDS_K * LB_LDS_K : 1];
    __shared__ uint32_t s_n[4];
    const int KK = K * K;
    if (LDS) {
        for (int i = threadIdx.x; i < KK; i += LB_THREADS) s_c[i] = 0u;
        __syncthreads();
    }
    uint32_t unseen = 0, skipped = 0;
    const size_t stride = (size_t)gridDim.x * LB_THREADS;
    for (size_t p = (size_t)blockIdx.x * LB_THREADS + threadIdx.x; p < HW; p += stride) {
        const uint32_t g = gt[p];
        const int32_t pr = pred[p];
        const bool on = (valid ? valid[p] != 0 : true) && g < (uint32_t)K;
        const bool seen = pr >= 0 && pr < K;                          // anything else counts as "no prediction": no index leaves K x K
        if (on && seen) {
            if (LDS) atomicAdd(&s_c[g * (uint32_t)K + (uint32_t)pr], 1u);
            else atomicAdd(&counts[(size_t)g * K + pr], 1u);
        }
        unseen += (on && !seen) ? 1u : 0u;
        skipped += on ? 0u : 1u;
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < KK; i += LB_THREADS) {
            const uint32_t c = s_c[i];
            if (c) atomicAdd(&counts[i], c);
        }
    }
    unseen = block_sum(unseen, s_n);
    __syncthreads();
    skipped = block_sum(skipped, s_n);
    if (threadIdx.x == 0) {
        if (unseen) atomicAdd(&side[0], unseen);
        if (skipped) atomicAdd(&side[1], skipped);
    }
}

// K by chunk: the smallest register chunk that holds it, the two-pass form beyond ("Label kernels")
#define MGS_LABEL_DISPATCH(VEC_, K_, LAUNCH)                                      \
    do {                                                                          \
        if ((K_) <= 8) { LAUNCH(VEC_, 8); }                                       \
        else if ((K_) <= 24) { LAUNCH(VEC_, 24); }                                \
        else { LAUNCH(VEC_, 0); }                                                 \
    } while (0)

static int launch_label_loss(const LabelArgs& a, void* scratch, hipStream_t s) {
    const size_t HW = (size_t)a.W * a.H;
    const bool vec = a.W % 4 == 0 && lb_al(a.feat, 16) && lb_al(a.d_feat, 16) && lb_al(a.labels, 16) && lb_al(a.valid, 16);
    const int nb = lb_blocks(vec ? HW / 4 : HW);
    double* part = (double*)((char*)scratch + LB_PART);
#define LB_LOSS(VEC_, KC_) hipLaunchKernelGGL((label_loss_kernel<VEC_, KC_>), dim3(nb), dim3(LB_THREADS), 0, s, a, part)
    if (vec) MGS_LABEL_DISPATCH(true, a.K, LB_LOSS);
    else MGS_LABEL_DISPATCH(false, a.K, LB_LOSS);
#undef LB_LOSS
    hipLaunchKernelGGL(label_finalize_kernel, dim3(1), dim3(LB_THREADS), 0, s, part, nb, a.count, (float*)scratch);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

static int label_size_error(const char* who, int32_t W, int32_t H, int32_t K) {
    if (W <= 0 || H <= 0) { set_error("%s: image size must be positive", who); return 1; }
    if ((size_t)W * H >= ((size_t)1 << 31)) { set_error("%s: width x height must stay below 2^31", who); return 1; }
    if (K < 1 || K > MGS_MAX_FEATURE_CHANNELS) { set_error("%s: K must be 1..%d", who, MGS_MAX_FEATURE_CHANNELS); return 1; }
    return 0;
}

size_t mgs_label_scratch_bytes(void) { return LB_PART + (size_t)LB_MAX_BLOCKS * sizeof(double); }

int mgs_label_prepare(int32_t W, int32_t H, int32_t K, const uint8_t* labels, const uint8_t* valid, void* scratch,
                      uint32_t* count_out, void* stream) {
    if (label_size_error("mgs_label_prepare", W, H, K)) return 1;
    if (!labels || !scratch || !count_out) { set_error("mgs_label_prepare: labels, scratch and count_out must be non-NULL"); return 1; }
    if (!lb_al(scratch, 8)) { set_error("mgs_label_prepare: scratch must be 8-byte aligned"); return 1; }
    const size_t HW = (size_t)W * H;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* part = (uint32_t*)((char*)scratch + LB_PART);
    const bool vec = W % 4 == 0 && lb_al(labels, 16) && lb_al(valid, 16);
    const int nb = lb_blocks(vec ? HW / 4 : HW);
    if (vec) hipLaunchKernelGGL(label_count_kernel<true>, dim3(nb), dim3(LB_THREADS), 0, s, labels, valid, K, HW, part);
    else hipLaunchKernelGGL(label_count_kernel<false>, dim3(nb), dim3(LB_THREADS), 0, s, labels, valid, K, HW, part);
    hipLaunchKernelGGL(label_count_finalize_kernel, dim3(1), dim3(LB_THREADS), 0, s, part, nb, (uint32_t)HW, count_out);
    MGS_HIP(hipGetLastError());
    return 0;
}

int mgs_label_loss_grads(int32_t W, int32_t H, int32_t K, const float* feat, const uint8_t* labels, const uint8_t* valid,
                         const uint32_t* count, void* scratch, float* d_feat, void* stream) {
    if (label_size_error("mgs_label_loss_grads", W, H, K)) return 1;
    if (!feat || !labels || !count || !scratch || !d_feat) {
        set_error("mgs_label_loss_grads: feat, labels, count, scratch and d_feat must be non-NULL");
        return 1;
    }
    if (!lb_al(scratch, 8)) { set_error("mgs_label_loss_grads: scratch must be 8-byte aligned"); return 1; }
    LabelArgs a;
    a.feat = feat; a.labels = labels; a.valid = valid; a.count = count; a.d_feat = d_feat;
    a.W = W; a.H = H; a.K = K;
    return launch_label_loss(a, scratch, (hipStream_t)stream);
}

int mgs_label_confusion(int32_t W, int32_t H, int32_t K, const int32_t* pred, const uint8_t* gt, const uint8_t* valid,
                        uint32_t* counts, uint32_t* side, void* stream) {
    if (label_size_error("mgs_label_confusion", W, H, K)) return 1;
    if (!pred || !gt || !counts || !side) { set_error("mgs_label_confusion: pred, gt, counts and side must be non-NULL"); return 1; }
    const size_t HW = (size_t)W * H;
    hipStream_t s = (hipStream_t)stream;
    // eight pixels per thread: a workgroup's flush of up to K x K counts is paid once per 2048 pixels at the least
    size_t nb = (HW + LB_THREADS * 8 - 1) / (LB_THREADS * 8);
    nb = nb < 1 ? 1 : (nb > 256 ? 256 : nb);
    if (K <= LB_LDS_K) hipLaunchKernelGGL(label_confusion_kernel<true>, dim3((unsigned)nb), dim3(LB_THREADS), 0, s, pred, gt, valid, K, HW, counts, side);
    else hipLaunchKernelGGL(label_confusion_kernel<false>, dim3((unsigned)nb), dim3(LB_THREADS), 0, s, pred, gt, valid, K, HW, counts, side);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
