// Depth hypothesis for a keyframe without measured depth (monocular operation): the image the back-projection reads in place
// of a sensor's, from the keyframe's frozen render.  [RECALL] of public upstream MonoGS' add_new_keyframe (the reference fork
// removed the code and kept its helper get_median_depth(..., return_std=True), /root/reference/utils/slam_utils.py:149-157, and
// rgb_boundary_threshold in every config): parity unpinned, checked against a float64 restatement (tests/monocular_mirror.py).
//
//   valid   = depth > 0 && opacity > opacity_min && valid_rgb
//   median  = lower median of depth[valid]                 (mgs_masked_median on the selected image: kfwindow.hip)
//   std     = unbiased standard deviation of depth[valid]  (two passes: the mean, then the squared deviations)
//   outlier = depth > median + std || depth < median - std || !valid          (both sums rounded to float32)
//   out     = (outlier ? median : depth) + noise * (outlier ? sigma_out : sigma_in) * std,   0 where !valid_rgb
//   init rule (no render, or fewer than two valid pixels): out = init_mean + init_sigma * noise,   0 where !valid_rgb
//
// One stream-ordered call, nine launches whatever the data: select (+ partial sums of the selected depths), the six launches of
// the median, the squared deviations, the elementwise result.  Every reduction is per-workgroup partials in double precision,
// added in a fixed order by whoever needs the total: no float atomics, nothing cleared, bitwise reproducible.  The caller
// brings the standard normals (no generator in the kernel).  HBM-bound: 9 B/pixel read + 4 written by the select, 4 by each
// median histogram pass and by the deviations, 13 read + 4 written by the result.
#include <math.h>

#include "common.h"

namespace mgs {

constexpr int PD_THREADS = 256;
constexpr int PD_MAX_WG = 256;              // workgroups of the two reductions (rows of partials)
constexpr int PD_PER_WG = 2048;             // elements a workgroup reduces before another one is worth its row
// scratch: [header 256 B: median float, count uint32][PD_MAX_WG doubles: sums][PD_MAX_WG doubles: squared deviations]
//          [n floats (rounded up to 256 B): the selected depths, 0 where !valid][mgs_median_scratch_bytes(n)]
constexpr size_t PD_HDR_BYTES = 256;
constexpr size_t PD_PART_BYTES = (size_t)PD_MAX_WG * sizeof(double);

static unsigned pd_workgroups(uint64_t n) {
    const uint64_t g = (n + PD_PER_WG - 1) / PD_PER_WG;
    return (unsigned)(g < 1 ? 1 : g > PD_MAX_WG ? PD_MAX_WG : g);
}
static size_t pd_sel_bytes(uint64_t n) { return align_up((size_t)n * sizeof(float), 256); }

struct PseudoDepthArgs {
    const float *depth, *opacity, *noise;
    const uint8_t* valid_rgb;
    float *sel, *out, *stats;
    double *part_sum, *part_dev;
    const float* median;
    const uint32_t* count;
    uint64_t n;
    int G;                                  // rows of partials the reductions wrote
    int use_render;                         // 0: the init rule for every pixel (no render was given)
    MgsPseudoDepthParams p;
};

// the workgroup's sum to its row of partials: wave sums by shuffles, the four waves' sums through LDS, ((w0 + w1) + (w2 + w3))
__device__ __forceinline__ void pd_store_partial(double v, double* __restrict__ row) {
    __shared__ double s_w[PD_THREADS / 64];
    v = block_sum(v, s_w);
    if (threadIdx.x == 0) row[blockIdx.x] = v;
}
// one wave adds the G partials in a fixed order, every lane gets the total
__device__ __forceinline__ double pd_sum_partials(const double* __restrict__ part, int G, int lane) {
    double v[1];
    wave_sum_rows(part, 1, G, lane, v);
    return v[0];
}

__device__ __forceinline__ float pd_select(const PseudoDepthArgs& a, float d, float op, bool rgb_ok) {
    return (d > 0.f && op > a.p.opacity_min && rgb_ok) ? d : 0.f;      // (a missing opacity image arrives as +inf)
}

// sel = valid ? depth : 0, and the workgroup's sum of the selected depths
template <bool VEC4>
__global__ void __launch_bounds__(PD_THREADS) pseudo_depth_select_kernel(PseudoDepthArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * PD_THREADS;
    double acc = 0.0;
    if (VEC4) {
        const uint64_t NQ = a.n / 4;
        for (uint64_t q = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x; q < NQ; q += stride) {
            const float4 d = ((const float4*)a.depth)[q];
            const float4 op = a.opacity ? ((const float4*)a.opacity)[q] : make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
            const uchar4 ok = a.valid_rgb ? ((const uchar4*)a.valid_rgb)[q] : make_uchar4(1, 1, 1, 1);
            float4 s;
            s.x = pd_select(a, d.x, op.x, ok.x != 0); s.y = pd_select(a, d.y, op.y, ok.y != 0);
            s.z = pd_select(a, d.z, op.z, ok.z != 0); s.w = pd_select(a, d.w, op.w, ok.w != 0);
            ((float4*)a.sel)[q] = s;
            acc += ((double)s.x + (double)s.y) + ((double)s.z + (double)s.w);
        }
    } else {
        for (uint64_t i = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x; i < a.n; i += stride) {
            const float s = pd_select(a, a.depth[i], a.opacity ? a.opacity[i] : INFINITY, a.valid_rgb ? a.valid_rgb[i] != 0 : true);
            a.sel[i] = s;
            acc += (double)s;
        }
    }
    pd_store_partial(acc, a.part_sum);
}

// the workgroup's sum of (d - mean)^2 over the selected depths; mean = (sum of the first pass's partials) / count
__global__ void __launch_bounds__(PD_THREADS) pseudo_depth_deviation_kernel(PseudoDepthArgs a) {
    __shared__ double s_mean;
    if (threadIdx.x < 64) {
        const double total = pd_sum_partials(a.part_sum, a.G, (int)threadIdx.x);
        if (threadIdx.x == 0) { const uint32_t c = a.count[0]; s_mean = c ? total / (double)c : 0.0; }
    }
    __syncthreads();
    const double mean = s_mean;
    const uint64_t stride = (uint64_t)gridDim.x * PD_THREADS;
    double acc = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x; i < a.n; i += stride) {
        const float s = a.sel[i];
        if (s > 0.f) { const double e = (double)s - mean; acc += e * e; }
    }
    pd_store_partial(acc, a.part_dev);
}

struct PdRule { float median, std, k_in, k_out, init_mean, init_sigma; bool init; };
__device__ __forceinline__ float pd_pixel(const PdRule& r, float d, float s, float z, bool rgb_ok) {
    if (!rgb_ok) return 0.f;
    if (r.init) return r.init_mean + r.init_sigma * z;
    const bool outlier = d > __fadd_rn(r.median, r.std) || d < __fsub_rn(r.median, r.std) || !(s > 0.f);
    return (outlier ? r.median : d) + z * (outlier ? r.k_out : r.k_in);
}

template <bool VEC4>
__global__ void __launch_bounds__(PD_THREADS) pseudo_depth_apply_kernel(PseudoDepthArgs a) {
    __shared__ float s_rule[2];
    __shared__ int s_init;
    if (threadIdx.x < 64) {
        // (every workgroup adds the partials up itself, in the same order: <= 2 KB out of L2 instead of one more launch)
        uint32_t c = 0;
        double ss = 0.0;
        if (a.use_render) {
            ss = pd_sum_partials(a.part_dev, a.G, (int)threadIdx.x);
            c = a.count[0];
        }
        if (threadIdx.x == 0) {
            const bool init = !a.use_render || c < 2u;                 // the unbiased deviation needs two samples
            const float med = init ? a.p.init_mean : a.median[0];
            const float sd = init ? a.p.init_sigma : (float)sqrt(ss / (double)(c - 1u));
            s_rule[0] = med; s_rule[1] = sd; s_init = init ? 1 : 0;
            if (blockIdx.x == 0) { a.stats[0] = med; a.stats[1] = sd; a.stats[2] = (float)c; a.stats[3] = init ? 1.f : 0.f; }
        }
    }
    __syncthreads();
    PdRule r;
    r.median = s_rule[0]; r.std = s_rule[1]; r.init = s_init != 0;
    r.k_in = a.p.sigma_in * r.std; r.k_out = a.p.sigma_out * r.std;
    r.init_mean = a.p.init_mean; r.init_sigma = a.p.init_sigma;
    const bool rd = a.use_render != 0;              // without a render neither `depth` nor `sel` exists
    const uint64_t stride = (uint64_t)gridDim.x * PD_THREADS;
    if (VEC4) {
        const uint64_t NQ = a.n / 4;
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint64_t q = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x; q < NQ; q += stride) {
            const float4 d = rd ? ((const float4*)a.depth)[q] : zero4, s = rd ? ((const float4*)a.sel)[q] : zero4;
            const float4 z = ((const float4*)a.noise)[q];
            const uchar4 ok = a.valid_rgb ? ((const uchar4*)a.valid_rgb)[q] : make_uchar4(1, 1, 1, 1);
            float4 o;
            o.x = pd_pixel(r, d.x, s.x, z.x, ok.x != 0); o.y = pd_pixel(r, d.y, s.y, z.y, ok.y != 0);
            o.z = pd_pixel(r, d.z, s.z, z.z, ok.z != 0); o.w = pd_pixel(r, d.w, s.w, z.w, ok.w != 0);
            ((float4*)a.out)[q] = o;
        }
    } else {
        for (uint64_t i = (uint64_t)blockIdx.x * PD_THREADS + threadIdx.x; i < a.n; i += stride)
            a.out[i] = pd_pixel(r, rd ? a.depth[i] : 0.f, rd ? a.sel[i] : 0.f, a.noise[i], a.valid_rgb ? a.valid_rgb[i] != 0 : true);
    }
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_pseudo_depth_scratch_bytes(uint64_t n) {
    return PD_HDR_BYTES + 2 * PD_PART_BYTES + pd_sel_bytes(n) + align_up(mgs_median_scratch_bytes(n), 256);
}

int mgs_pseudo_depth(int32_t W, int32_t H, const float* render_depth, const float* render_opacity, const uint8_t* valid_rgb,
                     const float* noise, const MgsPseudoDepthParams* p, void* scratch, float* depth_out, float* stats_out,
                     void* stream) {
    if (W <= 0 || H <= 0) { set_error("mgs_pseudo_depth: image size must be positive"); return 1; }
    if (!noise || !p || !depth_out || !stats_out) {
        set_error("mgs_pseudo_depth: noise, params, depth_out and stats_out must be non-NULL");
        return 1;
    }
    if (render_depth && (!scratch || ((size_t)scratch % 256) != 0)) {
        set_error("mgs_pseudo_depth: scratch must be non-NULL and 256-byte aligned when a render is given");
        return 1;
    }
    const uint64_t n = (uint64_t)W * (uint64_t)H;
    if (n >= ((uint64_t)1 << 32)) { set_error("mgs_pseudo_depth: W x H must stay below 2^32"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    PseudoDepthArgs a;
    a.depth = render_depth; a.opacity = render_depth ? render_opacity : nullptr; a.noise = noise; a.valid_rgb = valid_rgb;
    a.out = depth_out; a.stats = stats_out; a.n = n; a.p = *p;
    a.use_render = render_depth ? 1 : 0;
    a.G = (int)pd_workgroups(n);
    char* base = (char*)scratch;
    a.median = (const float*)base;
    a.count = (const uint32_t*)(base + sizeof(float));
    a.part_sum = (double*)(base + PD_HDR_BYTES);
    a.part_dev = (double*)(base + PD_HDR_BYTES + PD_PART_BYTES);
    a.sel = (float*)(base + PD_HDR_BYTES + 2 * PD_PART_BYTES);
    void* median_scratch = base + PD_HDR_BYTES + 2 * PD_PART_BYTES + pd_sel_bytes(n);
    auto al = [](const void* q, size_t m) { return q == nullptr || ((size_t)q % m) == 0; };
    const bool vec4 = n % 4 == 0 && al(render_depth, 16) && al(render_opacity, 16) && al(noise, 16) && al(depth_out, 16) &&
                      al(valid_rgb, 4);
    const uint64_t per = (uint64_t)PD_THREADS * 4;
    const uint64_t want = (n + per - 1) / per;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want > 2048 ? 2048 : want);
    if (a.use_render) {
        if (vec4) hipLaunchKernelGGL(pseudo_depth_select_kernel<true>, dim3(a.G), dim3(PD_THREADS), 0, s, a);
        else hipLaunchKernelGGL(pseudo_depth_select_kernel<false>, dim3(a.G), dim3(PD_THREADS), 0, s, a);
        // the selection holds 0 where a pixel does not count: the lower bound 0 is its mask
        const int rc = mgs_masked_median(a.sel, nullptr, n, 0.f, median_scratch, (float*)base, (uint32_t*)(base + sizeof(float)), s);
        if (rc) return rc;
        hipLaunchKernelGGL(pseudo_depth_deviation_kernel, dim3(a.G), dim3(PD_THREADS), 0, s, a);
    }
    if (vec4) hipLaunchKernelGGL(pseudo_depth_apply_kernel<true>, dim3(grid), dim3(PD_THREADS), 0, s, a);
    else hipLaunchKernelGGL(pseudo_depth_apply_kernel<false>, dim3(grid), dim3(PD_THREADS), 0, s, a);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
