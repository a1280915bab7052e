// Fused SSIM (Wang et al. 2004, the form every 3DGS code base uses), forward value + analytic gradient, and the fused
// colour-refinement loss (1 - lambda) L1 + lambda (1 - SSIM) that goes with it.
//
// Per plane (one channel of one image, H x W float32), g the normalised 11-tap Gaussian of sigma 1.5, applied separably with
// ZERO padding:
//   mu1 = g*x, mu2 = g*y, s11 = g*x^2 - mu1^2, s22 = g*y^2 - mu2^2, s12 = g*xy - mu1 mu2
//   map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2))
// "same": mean of the whole map; "valid": mean of the map without its outer 5 pixels.  Gradient with respect to x only.
//
// Forward: one 256-thread workgroup per 32 x 32 output tile of one plane.  The 42 x 42 haloed tile of both images goes to LDS,
// the horizontal pass runs from LDS through a 14-value register window (four outputs per thread) and its five statistics
// replace the inputs in the same LDS; the vertical pass slides a 14-row window down a column (four outputs per thread).
// With TRAIN it stores d map / d mu1 (total: through s11 and s12 as well), d map / d s11, d map / d s12 -- zero outside the
// averaged region -- as three planes.  Backward: the same separable window over those planes,
//   dL/dx = k (g*D_mu + 2 x g*D_s11 + y g*D_s12)  [+ k_l1 sgn(x - y) in the refinement loss].
// Sums: per-workgroup partials + a one-workgroup finalize that adds them in a fixed order.  No atomics: bitwise reproducible.
//
// Cancellation: s11 = g*x^2 - mu1^2 loses everything to rounding on a flat image (variance 1e-6 next to x^2 = 0.5).  The
// statistics are therefore accumulated around a per-tile origin m (the second image's value at the tile centre): with
// x' = x - m inside the image and 0 outside, a = g*x', q = weight of the window that falls outside the image, s0 = 1 - q,
//   mu1 = a1 + m s0,  s11 = g*x'^2 - a1^2 + q (2 m a1 + m^2 s0),  s12 = g*x'y' - a1 a2 + q (m (a1 + a2) + m^2 s0)
// which is the zero-padded definition exactly (q = 0 away from the border).
#include "common.h"

namespace mgs {

constexpr int SS_THREADS = 256;
constexpr int SS_T = 32;                    // tile side
constexpr int SS_R = 5;                     // window radius
constexpr int SS_HT = SS_T + 2 * SS_R;      // haloed tile side: 42
constexpr int SS_IS = SS_HT + 1;            // LDS row stride of the haloed inputs: odd, so the eight (row, quad) items of a
                                            // half-wave's four rows fall into 32 different banks
constexpr int SS_ITEMS = SS_HT * (SS_T / 4);   // horizontal pass: (row, four columns) items, 336 for 256 threads
constexpr int SS_WIN = 2 * SS_R + 4;        // inputs of four adjacent outputs: 14
enum : int { SS_LOSS = 0, SS_L1 = 1, SS_SSIM = 2, SS_HDR = 16 };   // scratch: 16 floats of results, partials, planes

__host__ __device__ constexpr float ssim_w(int k) {
    constexpr float g[11] = {0.00102838008f, 0.00759875814f, 0.0360007721f, 0.109360690f, 0.213005538f, 0.266011725f,
                             0.213005538f, 0.109360690f, 0.0360007721f, 0.00759875814f, 0.00102838008f};
    return g[k];
}

struct SsimArgs {
    const float *x, *y;
    int W, H, valid;
    float C1, C2;
};

__device__ __forceinline__ float ssim_sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// weight of the 11-tap window centred on p that falls outside [0, n)
__device__ __forceinline__ float ssim_outside(int p, int n) {
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < 11; ++t) {
        const int s = p + t - SS_R;
        q += (s < 0 || s >= n) ? ssim_w(t) : 0.f;
    }
    return q;
}

// one pixel of the map from its five shifted statistics (a1, a2, g*x'^2, g*y'^2, g*x'y'); returns its share of the sum and,
// with TRAIN, stores the three derivatives (zero where the pixel is not averaged).  BORDER = false: q = 0, nothing to correct.
// Reciprocals are v_rcp_f32 (1 ulp): the map's error stays ~1e-7, three orders under the bar, for a third of the
// epilogue's instructions.
template <bool TRAIN, bool BORDER>
__device__ __forceinline__ float ssim_pixel(const SsimArgs& a, const float st[5], float m, float q, bool counted,
                                            float* __restrict__ dplanes, size_t total, size_t p) {
    const float a1 = st[0], a2 = st[1];
    float mu1 = a1 + m, mu2 = a2 + m;
    float s11 = st[2] - a1 * a1, s22 = st[3] - a2 * a2, s12 = st[4] - a1 * a2;
    if (BORDER) {
        const float s0 = 1.f - q, mm = m * m * s0;
        mu1 = a1 + m * s0; mu2 = a2 + m * s0;
        s11 += q * (2.f * m * a1 + mm);
        s22 += q * (2.f * m * a2 + mm);
        s12 += q * (m * (a1 + a2) + mm);
    }
    const float A = mu1 * mu1 + mu2 * mu2 + a.C1, B = s11 + s22 + a.C2;
    const float N1 = 2.f * mu1 * mu2 + a.C1, N2 = 2.f * s12 + a.C2;
    const float rA = __builtin_amdgcn_rcpf(A), rB = __builtin_amdgcn_rcpf(B);
    const float inv = rA * rB;
    const float map = N1 * N2 * inv;
    if (TRAIN) {
        const float d11 = -map * rB;
        const float d12 = 2.f * N1 * inv;
        const float dmu = 2.f * N2 * inv * (mu2 - mu1 * N1 * rA) - 2.f * mu1 * d11 - mu2 * d12;
        dplanes[p] = counted ? dmu : 0.f;
        dplanes[total + p] = counted ? d11 : 0.f;
        dplanes[2 * total + p] = counted ? d12 : 0.f;
    }
    return counted ? map : 0.f;
}

template <bool TRAIN>
__global__ void __launch_bounds__(SS_THREADS) ssim_forward_kernel(SsimArgs a, float* __restrict__ part,
                                                                  float* __restrict__ dplanes, size_t total) {
    // haloed inputs [2][42][43] first, then the horizontal statistics [5][42][32] in the same memory
    __shared__ __align__(16) float s_buf[5 * SS_HT * SS_T];
    __shared__ float s_red[2][4];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
    const int W = a.W, H = a.H;
    const size_t base = (size_t)blockIdx.z * W * H;
    const float* __restrict__ X = a.x + base;
    const float* __restrict__ Y = a.y + base;
    float m = Y[(size_t)min(y0 + SS_T / 2, H - 1) * W + min(x0 + SS_T / 2, W - 1)];
    if (!(fabsf(m) <= 4.f)) m = 0.f;           // (a NaN or a wild pixel must not spread over the tile through the origin)

    float l1 = 0.f;
    for (int i = tid; i < SS_HT * SS_HT; i += SS_THREADS) {
        const int r = i / SS_HT, c = i - r * SS_HT;
        const int gy = y0 + r - SS_R, gx = x0 + c - SS_R;
        float xv = 0.f, yv = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float xr = X[(size_t)gy * W + gx], yr = Y[(size_t)gy * W + gx];
            xv = xr - m; yv = yr - m;
            if (r >= SS_R && r < SS_R + SS_T && c >= SS_R && c < SS_R + SS_T) l1 += fabsf(__fsub_rn(xr, yr));
        }
        s_buf[r * SS_IS + c] = xv;
        s_buf[SS_HT * SS_IS + r * SS_IS + c] = yv;
    }
    __syncthreads();

    // horizontal pass into registers (the statistics overwrite the inputs once every thread has read its own)
    float h[2][5][4];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int item = tid + it * SS_THREADS;
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
            for (int o = 0; o < 4; ++o) h[it][k][o] = 0.f;
        if (item < SS_ITEMS) {
            const int r = item >> 3, q = item & 7;
            const float* px = s_buf + r * SS_IS + 4 * q;
            const float* py = px + SS_HT * SS_IS;
#pragma unroll
            for (int j = 0; j < SS_WIN; ++j) {
                const float xv = px[j], yv = py[j];
                const float xx = xv * xv, yy = yv * yv, xy = xv * yv;
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const int t = j - o;
                    if (t >= 0 && t < 11) {
                        const float w = ssim_w(t);
                        h[it][0][o] = fmaf(w, xv, h[it][0][o]);
                        h[it][1][o] = fmaf(w, yv, h[it][1][o]);
                        h[it][2][o] = fmaf(w, xx, h[it][2][o]);
                        h[it][3][o] = fmaf(w, yy, h[it][3][o]);
                        h[it][4][o] = fmaf(w, xy, h[it][4][o]);
                    }
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int item = tid + it * SS_THREADS;
        if (item < SS_ITEMS) {
            const int r = item >> 3, q = item & 7;
#pragma unroll
            for (int k = 0; k < 5; ++k)      // 16-byte stores: the eight quads of a row are 128 contiguous bytes
                *reinterpret_cast<float4*>(s_buf + (k * SS_HT + r) * SS_T + 4 * q) =
                    make_float4(h[it][k][0], h[it][k][1], h[it][k][2], h[it][k][3]);
        }
    }
    __syncthreads();

    // vertical pass: column c, output rows 4 rb .. 4 rb + 3 (a half-wave reads one row: 32 consecutive banks)
    const int c = tid & 31, rb = tid >> 5;
    float v[5][4];
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int o = 0; o < 4; ++o) v[k][o] = 0.f;
#pragma unroll
    for (int j = 0; j < SS_WIN; ++j) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float s = s_buf[(k * SS_HT + 4 * rb + j) * SS_T + c];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int t = j - o;
                if (t >= 0 && t < 11) v[k][o] = fmaf(ssim_w(t), s, v[k][o]);
            }
        }
    }

    // interior tiles (every window inside the image, every pixel counted): q = 0, no bounds, no border weights
    const bool border = x0 < SS_R || y0 < SS_R || x0 + SS_T + SS_R > W || y0 + SS_T + SS_R > H;
    const int gx = x0 + c;
    float sum = 0.f;
    if (!border) {
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float st[5] = {v[0][o], v[1][o], v[2][o], v[3][o], v[4][o]};
            sum += ssim_pixel<TRAIN, false>(a, st, m, 0.f, true, dplanes, total, base + (size_t)(y0 + 4 * rb + o) * W + gx);
        }
    } else {
        const float qx = ssim_outside(gx, W);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int gy = y0 + 4 * rb + o;
            if (gx < W && gy < H) {
                const float qy = ssim_outside(gy, H);
                const bool counted = !a.valid || (gx >= SS_R && gx < W - SS_R && gy >= SS_R && gy < H - SS_R);
                const float st[5] = {v[0][o], v[1][o], v[2][o], v[3][o], v[4][o]};
                sum += ssim_pixel<TRAIN, true>(a, st, m, qx + qy - qx * qy, counted, dplanes, total, base + (size_t)gy * W + gx);
            }
        }
    }
    block_sum(sum, l1, s_red[0], s_red[1]);
    if (tid == 0) {
        const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part[2 * wg] = sum;
        part[2 * wg + 1] = l1;
    }
}

// one workgroup: thread t adds partials t, t + 256, ... in order, then the fixed tree of block_sum (wave_ops.h)
__global__ void __launch_bounds__(SS_THREADS) ssim_finalize_kernel(const float* __restrict__ part, int nwg, float count,
                                                                   float count_l1, float lambda, int refine,
                                                                   float* __restrict__ hdr, float* __restrict__ value_out) {
    __shared__ float s_red[2][4];
    float s = 0.f, l = 0.f;
    for (int b = threadIdx.x; b < nwg; b += SS_THREADS) { s += part[2 * (size_t)b]; l += part[2 * (size_t)b + 1]; }
    block_sum(s, l, s_red[0], s_red[1]);
    if (threadIdx.x == 0) {
        const float ssim = s / count, l1 = l / count_l1;
        const float loss = (1.f - lambda) * l1 + lambda * (1.f - ssim);
        hdr[SS_LOSS] = loss; hdr[SS_L1] = l1; hdr[SS_SSIM] = ssim;
        if (value_out) value_out[0] = refine ? loss : ssim;
    }
}

template <bool REFINE>
__global__ void __launch_bounds__(SS_THREADS) ssim_backward_kernel(SsimArgs a, const float* __restrict__ dplanes, size_t total,
                                                                   const float* __restrict__ grad_out, float k_ssim, float k_l1,
                                                                   float* __restrict__ out) {
    // haloed derivative planes [3][42][43] first, then their horizontal sums [3][42][32] in the same memory
    __shared__ __align__(16) float s_buf[3 * SS_HT * SS_IS];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
    const int W = a.W, H = a.H;
    const size_t base = (size_t)blockIdx.z * W * H;
    const float go = grad_out ? grad_out[0] : 1.f;
    const float ks = go * k_ssim, kl = go * k_l1;

    for (int i = tid; i < SS_HT * SS_HT; i += SS_THREADS) {
        const int r = i / SS_HT, c = i - r * SS_HT;
        const int gy = y0 + r - SS_R, gx = x0 + c - SS_R;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t p = base + (size_t)gy * W + gx;
            d0 = dplanes[p]; d1 = dplanes[total + p]; d2 = dplanes[2 * total + p];
        }
        s_buf[r * SS_IS + c] = d0;
        s_buf[SS_HT * SS_IS + r * SS_IS + c] = d1;
        s_buf[2 * SS_HT * SS_IS + r * SS_IS + c] = d2;
    }
    __syncthreads();

    float h[2][3][4];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int item = tid + it * SS_THREADS;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int o = 0; o < 4; ++o) h[it][k][o] = 0.f;
        if (item < SS_ITEMS) {
            const int r = item >> 3, q = item & 7;
            const float* p0 = s_buf + r * SS_IS + 4 * q;
#pragma unroll
            for (int j = 0; j < SS_WIN; ++j) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float s = p0[k * SS_HT * SS_IS + j];
#pragma unroll
                    for (int o = 0; o < 4; ++o) {
                        const int t = j - o;
                        if (t >= 0 && t < 11) h[it][k][o] = fmaf(ssim_w(t), s, h[it][k][o]);
                    }
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int item = tid + it * SS_THREADS;
        if (item < SS_ITEMS) {
            const int r = item >> 3, q = item & 7;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                *reinterpret_cast<float4*>(s_buf + (k * SS_HT + r) * SS_T + 4 * q) =
                    make_float4(h[it][k][0], h[it][k][1], h[it][k][2], h[it][k][3]);
        }
    }
    __syncthreads();

    const int c = tid & 31, rb = tid >> 5;
    float v[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int o = 0; o < 4; ++o) v[k][o] = 0.f;
#pragma unroll
    for (int j = 0; j < SS_WIN; ++j) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float s = s_buf[(k * SS_HT + 4 * rb + j) * SS_T + c];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int t = j - o;
                if (t >= 0 && t < 11) v[k][o] = fmaf(ssim_w(t), s, v[k][o]);
            }
        }
    }
    const int gx = x0 + c;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = y0 + 4 * rb + o;
        if (gx < W && gy < H) {
            const size_t p = base + (size_t)gy * W + gx;
            const float xv = a.x[p], yv = a.y[p];
            float g = ks * (v[0][o] + 2.f * xv * v[1][o] + yv * v[2][o]);
            if (REFINE) g += kl * ssim_sgn(__fsub_rn(xv, yv));
            out[p] = g;
        }
    }
}

static dim3 ssim_grid(const SsimArgs& a, int planes) {
    return dim3((a.W + SS_T - 1) / SS_T, (a.H + SS_T - 1) / SS_T, planes);
}
static size_t ssim_nwg(int planes, int W, int H) {
    return (size_t)((W + SS_T - 1) / SS_T) * ((H + SS_T - 1) / SS_T) * planes;
}
static size_t ssim_plane_offset(int planes, int W, int H) {       // in floats, 16-byte aligned
    return (SS_HDR + 2 * ssim_nwg(planes, W, H) + 3) & ~(size_t)3;
}
static double ssim_count(int planes, int W, int H, int valid) {
    return valid ? (double)planes * (W - 2 * SS_R) * (H - 2 * SS_R) : (double)planes * W * H;
}

// lambda < 0: plain SSIM (value_out = SSIM); otherwise the refinement loss (value_out = loss)
int launch_ssim_forward(const SsimArgs& a, int planes, int train, float lambda, float* scratch, float* value_out, hipStream_t s) {
    const size_t total = (size_t)planes * a.W * a.H;
    float* part = scratch + SS_HDR;
    float* dplanes = scratch + ssim_plane_offset(planes, a.W, a.H);
    if (train) hipLaunchKernelGGL(ssim_forward_kernel<true>, ssim_grid(a, planes), dim3(SS_THREADS), 0, s, a, part, dplanes, total);
    else hipLaunchKernelGGL(ssim_forward_kernel<false>, ssim_grid(a, planes), dim3(SS_THREADS), 0, s, a, part, (float*)nullptr, total);
    const int refine = lambda >= 0.f;
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3(1), dim3(SS_THREADS), 0, s, part, (int)ssim_nwg(planes, a.W, a.H),
                       (float)ssim_count(planes, a.W, a.H, a.valid), (float)((double)planes * a.W * a.H),
                       refine ? lambda : 0.f, refine, scratch, value_out);
    MGS_HIP(hipGetLastError());
    return 0;
}

int launch_ssim_backward(const SsimArgs& a, int planes, float lambda, const float* scratch, const float* grad_out, float* out,
                         hipStream_t s) {
    const size_t total = (size_t)planes * a.W * a.H;
    const float* dplanes = scratch + ssim_plane_offset(planes, a.W, a.H);
    const double n = ssim_count(planes, a.W, a.H, a.valid);
    if (lambda >= 0.f)
        hipLaunchKernelGGL(ssim_backward_kernel<true>, ssim_grid(a, planes), dim3(SS_THREADS), 0, s, a, dplanes, total, grad_out,
                           (float)(-(double)lambda / n), (float)((1.0 - (double)lambda) / (double)total), out);
    else
        hipLaunchKernelGGL(ssim_backward_kernel<false>, ssim_grid(a, planes), dim3(SS_THREADS), 0, s, a, dplanes, total, grad_out,
                           (float)(1.0 / n), 0.f, out);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

static int ssim_fill(SsimArgs& a, int32_t planes, int32_t W, int32_t H, int32_t valid, float C1, float C2, const float* img1,
                     const float* img2) {
    if (planes <= 0 || W <= 0 || H <= 0) { set_error("planes and image size must be positive"); return 1; }
    if (planes > 65535) { set_error("at most 65535 planes (batch x channels) per call"); return 1; }
    if ((size_t)planes * W * H >= ((size_t)1 << 31)) { set_error("planes x width x height must stay below 2^31"); return 1; }
    if (valid && (W < 2 * SS_R + 1 || H < 2 * SS_R + 1)) {
        set_error("padding \"valid\" needs an image of at least 11 x 11 pixels (the averaged region would be empty)");
        return 1;
    }
    if (!img1 || !img2) { set_error("img1 and img2 must be non-NULL"); return 1; }
    a.x = img1; a.y = img2; a.W = W; a.H = H; a.valid = valid ? 1 : 0; a.C1 = C1; a.C2 = C2;
    return 0;
}

size_t mgs_ssim_scratch_bytes(int32_t planes, int32_t W, int32_t H, int32_t train) {
    if (planes <= 0 || W <= 0 || H <= 0) return SS_HDR * sizeof(float);
    return (ssim_plane_offset(planes, W, H) + (train ? 3 * (size_t)planes * W * H : 0)) * sizeof(float);
}

int mgs_ssim_forward(int32_t planes, int32_t W, int32_t H, int32_t valid, int32_t train, float C1, float C2, const float* img1,
                     const float* img2, float* scratch, float* value_out, void* stream) {
    SsimArgs a;
    if (ssim_fill(a, planes, W, H, valid, C1, C2, img1, img2)) return 1;
    if (!scratch || !value_out) { set_error("scratch and value_out must be non-NULL"); return 1; }
    return launch_ssim_forward(a, planes, train, -1.f, scratch, value_out, (hipStream_t)stream);
}

int mgs_ssim_backward(int32_t planes, int32_t W, int32_t H, int32_t valid, float C1, float C2, const float* img1,
                      const float* img2, const float* scratch, const float* grad_out, float* d_img1, void* stream) {
    SsimArgs a;
    if (ssim_fill(a, planes, W, H, valid, C1, C2, img1, img2)) return 1;
    if (!scratch || !d_img1) { set_error("scratch and d_img1 must be non-NULL"); return 1; }
    return launch_ssim_backward(a, planes, -1.f, scratch, grad_out, d_img1, (hipStream_t)stream);
}

static int refine_fill(SsimArgs& a, int32_t W, int32_t H, float lambda_ssim, const float* render, const float* gt_rgb) {
    if (!(lambda_ssim >= 0.f && lambda_ssim <= 1.f)) { set_error("lambda_ssim must lie in [0, 1]"); return 1; }
    return ssim_fill(a, 3, W, H, 1, MGS_SSIM_C1, MGS_SSIM_C2, render, gt_rgb);
}

int mgs_refine_loss_forward(int32_t W, int32_t H, float lambda_ssim, const float* render, const float* gt_rgb, float* scratch,
                            float* loss_out, void* stream) {
    SsimArgs a;
    if (refine_fill(a, W, H, lambda_ssim, render, gt_rgb)) return 1;
    if (!scratch || !loss_out) { set_error("scratch and loss_out must be non-NULL"); return 1; }
    return launch_ssim_forward(a, 3, 1, lambda_ssim, scratch, loss_out, (hipStream_t)stream);
}

int mgs_refine_loss_backward(int32_t W, int32_t H, float lambda_ssim, const float* render, const float* gt_rgb,
                             const float* scratch, const float* grad_out, float* d_render, void* stream) {
    SsimArgs a;
    if (refine_fill(a, W, H, lambda_ssim, render, gt_rgb)) return 1;
    if (!scratch || !d_render) { set_error("scratch and d_render must be non-NULL"); return 1; }
    return launch_ssim_backward(a, 3, lambda_ssim, scratch, grad_out, d_render, (hipStream_t)stream);
}

int mgs_refine_loss_grads(int32_t W, int32_t H, float lambda_ssim, const float* render, const float* gt_rgb, float* scratch,
                          float* d_render, void* stream) {
    SsimArgs a;
    if (refine_fill(a, W, H, lambda_ssim, render, gt_rgb)) return 1;
    if (!scratch || !d_render) { set_error("scratch and d_render must be non-NULL"); return 1; }
    if (int rc = launch_ssim_forward(a, 3, 1, lambda_ssim, scratch, nullptr, (hipStream_t)stream)) return rc;
    return launch_ssim_backward(a, 3, lambda_ssim, scratch, nullptr, d_render, (hipStream_t)stream);
}

}  // extern "C"
