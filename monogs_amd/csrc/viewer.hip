// The headless viewer: what the reference's viewer window shows, as uint8 [H, W, 3] images on the device.
//
// Boundary replaced: viewer/slam_viewer.py there needs Open3D's GUI, GLFW and an OpenGL context; its five "shaders" are
//   rgb / segmentation   the rasteriser's colour image, clipped and truncated to bytes              (slam_viewer.py:600-603,767-768)
//   depth                jet(depth / max(depth))                                                    (:605-622)
//   time                 jet(opacity image)                                                         (:624-636)
//   elipsoids            gl_render with render_mod = -4: every splat an opaque ellipse              (gau_frag.glsl:20-35)
// and camera frustums / the trajectory are Open3D line sets drawn over that image.  Here: one walk kernel for the ellipsoids
// (through the tables of a finished forward, as features.hip), one line rasteriser with integer arithmetic only, and one compose
// kernel that turns a float image into bytes by the mode's rule and resolves the line overlay.  No kernel synchronises the
// host, none keeps state: everything may be captured in a hipGraph.
//
// ---- ellipsoid walk ------------------------------------------------------------------------------------------------------
// The reference's fragments have alpha 0 or 1 (alpha > 0.4 after the 0.99 cap) and are blended far to near: the NEAREST opaque
// fragment wins.  So pixel p shows colour[g] exp(power) of the first entry g of its tile's list, in blend order, with
// power <= 0 and min(0.99, opacity exp(power)) > threshold -- power and alpha formed by tile_walk.h's
// falloff, as the blend forward forms them -- and black (hit -1) where no entry qualifies.
// What is read: the blend records, the point list in blend order, the canonical tile ranges.  NOT n_contrib (a pixel
// saturated by many faint splats has its first opaque one behind the forward's stop) and NOT the forward's survivor masks
// (the forward never entered the steps behind its stop): the walk culls for itself, lane l testing the alpha >= 1/255 box of
// entry l of the step against the quadrant (threshold >= 1/255 is an argument check, so the box is conservative).
// gfx950 mapping (tile_walk.h): a 16x16 tile is one 256-thread workgroup whose four waves never synchronise; wave w
// owns the 8x8 quadrant (w & 1, w >> 1), one pixel per lane; a candidate's record arrives with scalar loads off the
// wave-uniform index (constant address space, common.h).  A wave retires once all its pixels have hit or the range ends.
#include "common.h"
#include "tile_walk.h"

#include <math.h>

namespace mgs {

namespace {

struct EllArgs {
    const float* __restrict__ rec;                  // [P][16]
    const uint32_t* __restrict__ point_list;
    const uint2* __restrict__ ranges;               // canonical: {0, 0} for an empty tile
    int W, H, gx;
    float threshold;
};

__global__ void __launch_bounds__(256) viewer_ellipsoids_kernel(EllArgs a, float* __restrict__ out, int32_t* __restrict__ hit) {
    const int tile = (int)blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    Quadrant q;
    MGS_QUADRANT_FILL(q, a, tile, wave, lane);
    // the quadrant's rectangle, grown by 0.05 px as the blend's cull has it (its own test, not quadrant_hit: the two round differently)
    const float qx_lo = (float)q.qx0i - 0.05f, qx_hi = (float)(q.qx0i + SUB - 1) + 0.05f;
    const float qy_lo = (float)q.qy0i - 0.05f, qy_hi = (float)(q.qy0i + SUB - 1) + 0.05f;
    const uint2 r = a.ranges[tile];
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.x), end = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.y);
    const const_float_p recs = MGS_CONST(a.rec);
    const float4* const rec4 = reinterpret_cast<const float4*>(a.rec);

    bool open = q.inside;                           // the pixel has no hit yet (a pixel outside the image never takes one)
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    int32_t h = -1;
    for (uint32_t base = first; base < end && __builtin_amdgcn_ballot_w64(open) != 0ull; base += WAVE) {
        const uint32_t i = base + (uint32_t)lane;
        uint32_t gid_l = 0u;
        float4 box = make_float4(0.f, 0.f, -1.f, -1.f);
        if (i < end) {
            gid_l = a.point_list[i];
            box = rec4[(size_t)gid_l * 4];           // {px, py, ex, ey}: outside px +- ex, py +- ey alpha < 1/255
        }
        const bool cand = box.z >= 0.f && box.x + box.z >= qx_lo && box.x - box.z <= qx_hi && box.y + box.w >= qy_lo &&
                          box.y - box.w <= qy_hi;
        unsigned long long mask = __builtin_amdgcn_ballot_w64(cand);
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            const uint32_t gid = bcast(gid_l, j);
            const const_float_p g = recs + (size_t)gid * REC_FLOATS;
            const float dx = g[R_X] - q.pxf, dy = g[R_Y] - q.pyf;
            const float power = falloff_power(dx, dy, g[R_CA], g[R_CB], g[R_CC]);
            const float G = __builtin_amdgcn_exp2f(power);
            const float alpha = falloff_alpha(g[R_OPAC], G);
            const bool take = open && !(power > 0.f) && alpha > a.threshold;
            if (__builtin_amdgcn_ballot_w64(take) == 0ull) continue;
            if (take) {
                c0 = g[R_R] * G, c1 = g[R_G] * G, c2 = g[R_B] * G;
                h = (int32_t)gid;
                open = false;
            }
            if (__builtin_amdgcn_ballot_w64(open) == 0ull) break;
        }
    }
    if (q.inside) {
        const size_t HW = (size_t)a.H * a.W;
        out[q.pix] = c0;
        out[HW + q.pix] = c1;
        out[2 * HW + q.pix] = c2;
        if (hit) hit[q.pix] = h;
    }
}

// no Gaussians: black, no hit anywhere
__global__ void __launch_bounds__(256) viewer_empty_kernel(float* __restrict__ out, int32_t* __restrict__ hit, size_t HW) {
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t i = i0; i < 3 * HW; i += stride) out[i] = 0.f;
    if (hit)
        for (size_t i = i0; i < HW; i += stride) hit[i] = -1;
}

// ---- line overlay ---------------------------------------------------------------------------------------------------------
// A segment is {x0, y0, x1, y1} in 1/16 pixel (pixel centres at multiples of 16), clipped by the host.  One 64-thread
// workgroup per segment: the major axis is the one with the larger extent (x on a tie); every integer pixel position m on it
// inside the segment gets the pixel whose minor coordinate is the segment's there, rounded half up:
//     n = floor((n0 dm + (n1 - n0)(16 m - m0) + 8 dm) / (16 dm)),  dm = m1 - m0 > 0,  in 64-bit integers.
// A segment that holds no such position lies within one pixel and paints the pixel its first endpoint rounds to (half up).
// owner[p] = max over the segments painting p of (index + 1): the highest index wins, whatever the order of the atomics.
__device__ __forceinline__ long long floor_div(long long a, long long b) {      // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

__global__ void __launch_bounds__(64) viewer_lines_kernel(const int32_t* __restrict__ segs, int S, int32_t* __restrict__ owner,
                                                          int W, int H) {
    const int s = (int)blockIdx.x;
    if (s >= S) return;
    const long long x0 = segs[4 * s], y0 = segs[4 * s + 1], x1 = segs[4 * s + 2], y1 = segs[4 * s + 3];
    const long long adx = x1 > x0 ? x1 - x0 : x0 - x1, ady = y1 > y0 ? y1 - y0 : y0 - y1;
    const bool xmajor = adx >= ady;
    long long m0 = xmajor ? x0 : y0, m1 = xmajor ? x1 : y1, n0 = xmajor ? y0 : x0, n1 = xmajor ? y1 : x1;
    if (m0 > m1) {
        long long t = m0; m0 = m1; m1 = t;
        t = n0; n0 = n1; n1 = t;
    }
    const long long dm = m1 - m0;
    const long long lim_m = xmajor ? W : H, lim_n = xmajor ? H : W;
    long long lo = -floor_div(-m0, 16), hi = floor_div(m1, 16);          // ceil(m0 / 16) .. floor(m1 / 16)
    if (dm == 0 || lo > hi) {
        if (threadIdx.x == 0) {
            const long long px = floor_div(x0 + 8, 16), py = floor_div(y0 + 8, 16);
            if (px >= 0 && px < W && py >= 0 && py < H) atomicMax(owner + (size_t)py * W + (size_t)px, s + 1);
        }
        return;
    }
    if (lo < 0) lo = 0;
    if (hi > lim_m - 1) hi = lim_m - 1;                                  // never steps outside the image, whatever the input
    for (long long m = lo + (long long)threadIdx.x; m <= hi; m += 64) {
        const long long n = floor_div(n0 * dm + (n1 - n0) * (16 * m - m0) + 8 * dm, 16 * dm);
        if (n < 0 || n >= lim_n) continue;
        const long long px = xmajor ? m : n, py = xmajor ? n : m;
        atomicMax(owner + (size_t)py * W + (size_t)px, s + 1);
    }
}

// ---- compose ----------------------------------------------------------------------------------------------------------------
// depth: the maximum of the depth image as float bits (the values are >= 0: the integer order of the bits is the float order;
// a negative value or a NaN counts as 0), reduced per wave, one atomic per wave.  The word was zeroed by the launcher.
__global__ void __launch_bounds__(256) viewer_max_kernel(const float* __restrict__ src, size_t n, uint32_t* __restrict__ word) {
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    uint32_t m = 0u;
    for (size_t i = i0; i < n; i += stride) {
        const float v = src[i];
        m = max(m, v > 0.f ? __float_as_uint(v) : 0u);
    }
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(word, m);
}

__device__ __forceinline__ float clip01(float c) { return fminf(fmaxf(c, 0.f), 1.f); }

// index into the 256-entry table as matplotlib takes it: clamp(floor(x * 256), 0, 255); -1 for a NaN (its "bad" colour: black)
__device__ __forceinline__ int jet_index(float x) {
    if (x != x) return -1;
    const float f = floorf(__fmul_rn(x, 256.f));
    return f < 0.f ? 0 : (f > 255.f ? 255 : (int)f);
}

__global__ void __launch_bounds__(256) viewer_compose_kernel(int mode, const float* __restrict__ src, size_t HW,
                                                             const uint8_t* __restrict__ lut, const uint32_t* __restrict__ max_word,
                                                             const int32_t* __restrict__ owner, const uint8_t* __restrict__ seg_rgb,
                                                             int n_segments, uint8_t* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    uint8_t r, g, b;
    const int32_t own = owner ? owner[p] : 0;
    if (own > 0 && own <= n_segments) {                       // the overlay: no depth test, the highest segment index
        const uint8_t* c = seg_rgb + (size_t)(own - 1) * 3;
        r = c[0], g = c[1], b = c[2];
    } else if (mode == MGS_VIEWER_RGB) {                      // torch.clip(c, 0, 1) * 255 -> .byte()
        r = (uint8_t)(int)__fmul_rn(clip01(src[p]), 255.f);
        g = (uint8_t)(int)__fmul_rn(clip01(src[HW + p]), 255.f);
        b = (uint8_t)(int)__fmul_rn(clip01(src[2 * HW + p]), 255.f);
    } else if (mode == MGS_VIEWER_ELLIPSOIDS) {               // GL's float -> unorm8: floor(clip(c) * 255 + 0.5), two roundings
        r = (uint8_t)(int)floorf(__fadd_rn(__fmul_rn(clip01(src[p]), 255.f), 0.5f));
        g = (uint8_t)(int)floorf(__fadd_rn(__fmul_rn(clip01(src[HW + p]), 255.f), 0.5f));
        b = (uint8_t)(int)floorf(__fadd_rn(__fmul_rn(clip01(src[2 * HW + p]), 255.f), 0.5f));
    } else {                                                  // depth (normalised by its maximum unless that is 0), time
        float x = src[p];
        if (mode == MGS_VIEWER_DEPTH) {
            const float mx = __uint_as_float(*max_word);
            if (mx != 0.f) x = __fdiv_rn(x, mx);
        }
        const int k = jet_index(x);
        r = g = b = 0;
        if (k >= 0) r = lut[3 * k], g = lut[3 * k + 1], b = lut[3 * k + 2];
    }
    out[3 * p] = r, out[3 * p + 1] = g, out[3 * p + 2] = b;
}

inline unsigned blocks_for(size_t n, size_t cap = 4096) {
    const size_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

int launch_viewer_ellipsoids(const mgs_camera& cam, int P, const GeometryState& g, const BinningState& b, const ImageState& img,
                             float threshold, float* out, int32_t* hit, hipStream_t s) {
    const int W = cam.image_width, H = cam.image_height;
    const int ntiles = tiles_x(W) * tiles_y(H);
    if (P == 0) {
        const size_t HW = (size_t)W * H;
        hipLaunchKernelGGL(viewer_empty_kernel, dim3(blocks_for(3 * HW)), dim3(256), 0, s, out, hit, HW);
        MGS_HIP(hipGetLastError());
        return 0;
    }
    EllArgs a;
    a.rec = g.rec;
    a.point_list = b.vals_sorted;
    a.ranges = img.ranges;
    a.W = W, a.H = H, a.gx = tiles_x(W);
    a.threshold = threshold;
    hipLaunchKernelGGL(viewer_ellipsoids_kernel, dim3(ntiles), dim3(256), 0, s, a, out, hit);
    MGS_HIP(hipGetLastError());
    return 0;
}

// scratch: [0] the depth maximum's word, [VIEWER_OWNER_OFFSET ..) the owner image of the overlay, int32 [H, W]
constexpr size_t VIEWER_OWNER_OFFSET = 256;
size_t viewer_scratch_bytes(int W, int H) { return VIEWER_OWNER_OFFSET + align_up((size_t)W * H * sizeof(int32_t), 256); }

int launch_viewer_lines(int W, int H, const int32_t* segs, int S, void* scratch, hipStream_t s) {
    int32_t* const owner = reinterpret_cast<int32_t*>((char*)scratch + VIEWER_OWNER_OFFSET);
    MGS_HIP(zero_fill(owner, (size_t)W * H * sizeof(int32_t), s));             // a kernel, not a memset node (common.h)
    if (S == 0) return 0;
    hipLaunchKernelGGL(viewer_lines_kernel, dim3(S), dim3(64), 0, s, segs, S, owner, W, H);
    MGS_HIP(hipGetLastError());
    return 0;
}

int launch_viewer_compose(int mode, int W, int H, const float* src, const uint8_t* lut, const uint8_t* seg_rgb, int S,
                          void* scratch, uint8_t* out, hipStream_t s) {
    const size_t HW = (size_t)W * H;
    uint32_t* const word = reinterpret_cast<uint32_t*>(scratch);
    const int32_t* const owner = S > 0 ? reinterpret_cast<const int32_t*>((char*)scratch + VIEWER_OWNER_OFFSET) : nullptr;
    if (mode == MGS_VIEWER_DEPTH) {
        MGS_HIP(zero_fill(word, sizeof(uint32_t), s));
        hipLaunchKernelGGL(viewer_max_kernel, dim3(blocks_for(HW, 256)), dim3(256), 0, s, src, HW, word);
        MGS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(viewer_compose_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, s, mode, src, HW, lut, word, owner,
                       seg_rgb, S, out);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // namespace mgs
