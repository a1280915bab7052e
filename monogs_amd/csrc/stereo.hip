// Stereo depth: what StereoDataset.__getitem__ (/root/reference/utils/dataset.py:595-629) does to a pair of grey images, on
// the device: rectify (optional), semi-global matching over D <= 64 disparities (five path directions), disparity -> depth.
// The algorithm is specified step by step in include/monogs_raster.h (mgs_stereo_depth); this file follows that numbering.
// All arithmetic up to the disparity image is integer and bit-exact against tests/stereo_mirror.py.
//
//   prepare    rectified 8-bit left / right (integer bilinear remap, or a copy), rgb_out = float32(double(g) / 255.0)
//   prefilter  per pixel and image the Birchfield-Tomasi triples (u, min, max over the half-pixel interval) of the x-Sobel
//              image P and of the grey image I, packed 3 x 8 bits per word                                     (steps 1, 2)
//   hsum       row sums of the pixel cost over 2s+1 clamped columns, a sliding window of ST_CHUNK outputs per thread,
//              uint16 [H][W-D][D]                                                                               (steps 2, 3)
//   vsum       column sums of those over 2s+1 clamped rows: the cost volume C, uint32 [H][W-D][D]               (step 3)
//   path x 5   one wave per path, one disparity per lane; L(q, d-1) and L(q, d+1) by wave shifts on the DPP data path, the
//              minimum over d by a DPP reduction, the loads of the next ST_UNROLL steps in flight while this block's
//              dependent chain runs.  The first direction writes S, the other four add to it (stream order: no atomics)
//   winner     one wave per pixel: (S << 6 | d) minimised over the wave gives the lowest best d, the uniqueness vote is a
//              ballot, the sub-pixel neighbours come by ds_bpermute                                              (step 5)
//   table      the right-view table of step 5 as a gather: thread (y, x2) scans its D candidate columns x2 + d in
//              ascending x and keeps the last minimum -- the sequential rule's "largest x among equal costs"
//   finish     left-right check of the nine neighbours, 3x3 median, depth                                    (steps 6, 7, 8)
// Twelve launches.  Every loop bound is a launch parameter, no kernel waits for another workgroup, no atomics, no LDS.
//
// Widths, from the bounds the entry point enforces (window 2s+1 <= 63, ftzero <= 127, P1, P2 <= 2^20):
//   pixel cost <= 2 ftzero + 255 <= 509;  row sum <= 63 x 509 = 32 067 (uint16);  C <= 63^2 x 509 = 2 020 221 (uint32);
//   L_r <= C + P2;  S <= 5 (C + P2) < 2^24, so (S << 6 | d) fits 30 bits and S x 100 fits 31.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace mgs {

constexpr int ST_THREADS = 256;
constexpr int ST_CHUNK = 16;          // outputs per thread of the two sliding-window kernels
constexpr int ST_UNROLL = 8;          // path steps per block of loads
constexpr uint32_t ST_INF = 0x3fffffffu;   // "+infinity" of the path recurrence: INF + P1 does not wrap

struct StereoDims {
    int W, H, D, W1;                  // W1 = W - D valid columns
};

// ---- prepare -----------------------------------------------------------------------------------------------------------------
// one grey pixel of the 8-bit remap (ingest.hip, ig_remap): 1/32-pixel coordinates, weights summing to 2^15, zero border; the
// coordinate is tested as a float before it is converted, a tap is read only inside the image
__device__ __forceinline__ uint32_t st_remap(const uint8_t* __restrict__ src, int W, int H, float mx, float my) {
    const float fx = rintf(mx * 32.0f), fy = rintf(my * 32.0f);
    if (!(fx >= -32.0f && fx < 32.0f * (float)W && fy >= -32.0f && fy < 32.0f * (float)H)) return 0;
    const int sx = (int)fx, sy = (int)fy;
    const int ix = sx >> 5, iy = sy >> 5;
    const uint32_t ax = (uint32_t)(sx & 31), ay = (uint32_t)(sy & 31);
    const bool x0 = ix >= 0, x1 = ix + 1 < W, y0 = iy >= 0, y1 = iy + 1 < H;
    uint32_t acc = 16384;
    if (y0 && x0) acc += (32 - ax) * (32 - ay) * 32 * src[(size_t)iy * W + ix];
    if (y0 && x1) acc += ax * (32 - ay) * 32 * src[(size_t)iy * W + ix + 1];
    if (y1 && x0) acc += (32 - ax) * ay * 32 * src[(size_t)(iy + 1) * W + ix];
    if (y1 && x1) acc += ax * ay * 32 * src[(size_t)(iy + 1) * W + ix + 1];
    return acc >> 15;
}

struct StereoPrepareArgs {
    const uint8_t *left, *right;
    const float *map_lx, *map_ly, *map_rx, *map_ry;
    uint8_t *rect_l, *rect_r;
    float* rgb_out;
    int W, H;
};

template <bool REMAP>
__global__ void __launch_bounds__(ST_THREADS) stereo_prepare_kernel(const StereoPrepareArgs a) {
    const size_t HW = (size_t)a.W * a.H;
    const size_t t = (size_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (t >= HW) return;
    uint32_t gl, gr;
    if (REMAP) {
        gl = st_remap(a.left, a.W, a.H, a.map_lx[t], a.map_ly[t]);
        gr = st_remap(a.right, a.W, a.H, a.map_rx[t], a.map_ry[t]);
    } else {
        gl = a.left[t]; gr = a.right[t];
    }
    a.rect_l[t] = (uint8_t)gl; a.rect_r[t] = (uint8_t)gr;
    const float c = (float)((double)gl / 255.0);
    a.rgb_out[t] = c; a.rgb_out[HW + t] = c; a.rgb_out[2 * HW + t] = c;
}

// ---- prefilter + Birchfield-Tomasi triples (steps 1, 2) ----------------------------------------------------------------------
__device__ __forceinline__ int st_sobel(const uint8_t* __restrict__ r0, const uint8_t* __restrict__ r1,
                                        const uint8_t* __restrict__ r2, int x, int W, int ftzero) {
    if (x == 0 || x == W - 1) return ftzero;
    const int g = ((int)r0[x + 1] - (int)r0[x - 1]) + 2 * ((int)r1[x + 1] - (int)r1[x - 1]) + ((int)r2[x + 1] - (int)r2[x - 1]);
    return min(max(g, -ftzero), ftzero) + ftzero;
}

__device__ __forceinline__ uint32_t st_triple(int l, int u, int r) {
    const int ul = (u + l) >> 1, ur = (u + r) >> 1;
    return (uint32_t)u | ((uint32_t)min(min(ul, ur), u) << 8) | ((uint32_t)max(max(ul, ur), u) << 16);
}

// trip[y][x] = {triple of P, triple of I}: byte 0 the value, byte 1 the interval's minimum, byte 2 its maximum
__device__ __forceinline__ uint2 st_triples(const uint8_t* __restrict__ img, int x, int y, int W, int H, int ftzero) {
    const uint8_t* r0 = img + (size_t)max(y - 1, 0) * W;
    const uint8_t* r1 = img + (size_t)y * W;
    const uint8_t* r2 = img + (size_t)min(y + 1, H - 1) * W;
    const int xl = max(x - 1, 0), xr = min(x + 1, W - 1);
    const int pu = st_sobel(r0, r1, r2, x, W, ftzero);
    return make_uint2(st_triple(st_sobel(r0, r1, r2, xl, W, ftzero), pu, st_sobel(r0, r1, r2, xr, W, ftzero)),
                      st_triple(r1[xl], r1[x], r1[xr]));
}

__global__ void __launch_bounds__(ST_THREADS) stereo_prefilter_kernel(const uint8_t* __restrict__ rect_l,
                                                                      const uint8_t* __restrict__ rect_r, int W, int H,
                                                                      int ftzero, uint2* __restrict__ trip_l,
                                                                      uint2* __restrict__ trip_r) {
    const size_t t = (size_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (t >= (size_t)W * H) return;
    const int y = (int)(t / W), x = (int)(t % W);
    trip_l[t] = st_triples(rect_l, x, y, W, H, ftzero);
    trip_r[t] = st_triples(rect_r, x, y, W, H, ftzero);
}

__device__ __forceinline__ int st_bt(uint32_t l, uint32_t r) {
    const int u = l & 255, u0 = (l >> 8) & 255, u1 = (l >> 16) & 255;
    const int v = r & 255, v0 = (r >> 8) & 255, v1 = (r >> 16) & 255;
    const int c0 = max(0, max(u - v1, v0 - u)), c1 = max(0, max(v - u1, u0 - v));
    return min(c0, c1);
}

// pixel cost of left column D + xv (xv already clamped to [0, W1)) against right column D + xv - d of the same row
__device__ __forceinline__ int st_pc(const uint2* __restrict__ tl, const uint2* __restrict__ tr, int D, int xv, int d) {
    const uint2 l = tl[D + xv], r = tr[D + xv - d];
    return st_bt(l.x, r.x) + st_bt(l.y, r.y);
}

// ---- window sums (step 3) ----------------------------------------------------------------------------------------------------
// thread = (row, chunk of ST_CHUNK valid columns, d), d fastest: row sums over the 2s+1 clamped columns around each
__global__ void __launch_bounds__(ST_THREADS) stereo_hsum_kernel(const uint2* __restrict__ trip_l, const uint2* __restrict__ trip_r,
                                                                 StereoDims dm, int s, int n_chunks, uint16_t* __restrict__ hs) {
    const size_t t = (size_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (t >= (size_t)dm.H * n_chunks * dm.D) return;
    const int d = (int)(t % dm.D);
    const int chunk = (int)((t / dm.D) % n_chunks);
    const int y = (int)(t / ((size_t)dm.D * n_chunks));
    const uint2* tl = trip_l + (size_t)y * dm.W;
    const uint2* tr = trip_r + (size_t)y * dm.W;
    const int xs = chunk * ST_CHUNK, xe = min(xs + ST_CHUNK, dm.W1), last = dm.W1 - 1;
    int sum = 0;
    for (int dx = -s; dx <= s; ++dx) sum += st_pc(tl, tr, dm.D, min(max(xs + dx, 0), last), d);
    uint16_t* out = hs + ((size_t)y * dm.W1) * dm.D + d;
    out[(size_t)xs * dm.D] = (uint16_t)sum;
    for (int x = xs + 1; x < xe; ++x) {
        sum += st_pc(tl, tr, dm.D, min(x + s, last), d) - st_pc(tl, tr, dm.D, max(x - s - 1, 0), d);
        out[(size_t)x * dm.D] = (uint16_t)sum;
    }
}

// thread = (chunk of ST_CHUNK rows, j = (valid column, d) flattened), j fastest: C = column sums over 2s+1 clamped rows
__global__ void __launch_bounds__(ST_THREADS) stereo_vsum_kernel(const uint16_t* __restrict__ hs, StereoDims dm, int s,
                                                                 int n_chunks, uint32_t* __restrict__ cost) {
    const size_t row = (size_t)dm.W1 * dm.D;
    const size_t t = (size_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (t >= row * n_chunks) return;
    const size_t j = t % row;
    const int chunk = (int)(t / row);
    const int ys = chunk * ST_CHUNK, ye = min(ys + ST_CHUNK, dm.H), last = dm.H - 1;
    uint32_t sum = 0;
    for (int dy = -s; dy <= s; ++dy) sum += hs[(size_t)min(max(ys + dy, 0), last) * row + j];
    cost[(size_t)ys * row + j] = sum;
    for (int y = ys + 1; y < ye; ++y) {
        sum += hs[(size_t)min(y + s, last) * row + j];
        sum -= hs[(size_t)max(y - s - 1, 0) * row + j];
        cost[(size_t)y * row + j] = sum;
    }
}

// ---- path aggregation (step 4) -----------------------------------------------------------------------------------------------
// Directions: 0 from the left, 1 from up-left, 2 from above, 3 from up-right, 4 from the right.  A path is the maximal run of
// valid pixels along its direction; path k < W1 (directions 1..3) starts in the top row at column k, the others on the side
// edge the direction enters through, at row k - W1 + 1.
template <int DIR, bool ADD>
__global__ void __launch_bounds__(ST_THREADS) stereo_path_kernel(const uint32_t* __restrict__ cost, uint32_t* __restrict__ sum,
                                                                 StereoDims dm, uint32_t P1, uint32_t P2, int n_paths) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6);
    if (k >= n_paths) return;                        // (wave-uniform: every lane of a running wave stays active)
    constexpr int DX = DIR == 0 || DIR == 1 ? 1 : (DIR == 2 ? 0 : -1), DY = DIR == 0 || DIR == 4 ? 0 : 1;
    int x0, y0, len;
    if (DIR == 0) { x0 = 0; y0 = k; len = dm.W1; }
    else if (DIR == 4) { x0 = dm.W1 - 1; y0 = k; len = dm.W1; }
    else if (DIR == 2) { x0 = k; y0 = 0; len = dm.H; }
    else {
        const bool top = k < dm.W1;
        x0 = top ? k : (DIR == 1 ? 0 : dm.W1 - 1);
        y0 = top ? 0 : k - dm.W1 + 1;
        len = min(DIR == 1 ? dm.W1 - x0 : x0 + 1, dm.H - y0);
    }
    const bool live = lane < dm.D;
    const long long step = ((long long)DY * dm.W1 + DX) * dm.D;
    const size_t base = ((size_t)y0 * dm.W1 + x0) * dm.D + (live ? lane : 0);
    const uint32_t* cp = cost + base;
    uint32_t* sp = sum + base;

    uint32_t cn[ST_UNROLL], sn[ST_UNROLL];
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) {
        const bool in = live && u < len;
        cn[u] = in ? cp[(long long)u * step] : 0u;
        sn[u] = (ADD && in) ? sp[(long long)u * step] : 0u;
    }
    uint32_t L = live ? 0u : ST_INF;                 // a predecessor outside the valid region has L = 0: the path starts with C
    for (int i = 0; i < len; i += ST_UNROLL) {
        uint32_t c[ST_UNROLL], sv[ST_UNROLL];
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) { c[u] = cn[u]; sv[u] = sn[u]; }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {        // the next block's loads, issued before this block's dependent chain
            const int n = i + ST_UNROLL + u;
            const bool in = live && n < len;
            cn[u] = in ? cp[(long long)n * step] : 0u;
            sn[u] = (ADD && in) ? sp[(long long)n * step] : 0u;
        }
#pragma unroll
        for (int u = 0; u < ST_UNROLL; ++u) {
            if (i + u < len) {                       // (wave-uniform)
                const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)ST_INF, (int)L, 0x138, 0xf, 0xf, false);   // wave_shr:1: L(q, d-1)
                const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)ST_INF, (int)L, 0x130, 0xf, 0xf, false);   // wave_shl:1: L(q, d+1)
                const uint32_t m = wave_min_dpp(L);
                const uint32_t best = min(min(L, m + P2), min(lo, hi) + P1);
                L = live ? c[u] + best - m : ST_INF;
                if (live) sp[(long long)(i + u) * step] = sv[u] + L;
            }
        }
    }
}

// ---- winner (step 5) ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ST_THREADS) stereo_winner_kernel(const uint32_t* __restrict__ sum, StereoDims dm, int uniq,
                                                                   size_t n_pix, int32_t* __restrict__ min_s,
                                                                   int16_t* __restrict__ best_d, int16_t* __restrict__ d16) {
    const int lane = threadIdx.x & 63;
    const size_t p = (size_t)blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6);
    if (p >= n_pix) return;                          // (wave-uniform)
    const bool live = lane < dm.D;
    const uint32_t s = live ? sum[p * dm.D + lane] : 0u;
    const uint32_t kmin = wave_min_dpp(live ? (s << 6) | (uint32_t)lane : 0xffffffffu);
    const int best = (int)(kmin & 63u);
    const int ms = (int)(kmin >> 6);
    const bool bad = live && (int)s * (100 - uniq) < ms * 100 && abs(best - lane) > 1;
    const bool invalid = __ballot(bad) != 0ull;
    const int sm = __shfl((int)s, max(best - 1, 0)), sq = __shfl((int)s, min(best + 1, dm.D - 1));
    if (lane == 0) {
        int v = -16;
        if (!invalid) {
            v = 16 * best;
            if (best > 0 && best < dm.D - 1) {
                const int den = max(sm + sq - 2 * ms, 1);
                v += ((sm - sq) * 16 + den) / (2 * den);            // truncates toward zero
            }
        }
        d16[p] = (int16_t)v;
        best_d[p] = (int16_t)(invalid ? -1 : best);
        min_s[p] = ms;
    }
}

// the right-view table: disp2[y][x2] over x2 in [0, W)
__global__ void __launch_bounds__(ST_THREADS) stereo_table_kernel(const int32_t* __restrict__ min_s, const int16_t* __restrict__ best_d,
                                                                  StereoDims dm, int16_t* __restrict__ disp2) {
    const size_t t = (size_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (t >= (size_t)dm.W * dm.H) return;
    const int y = (int)(t / dm.W), x2 = (int)(t % dm.W);
    const size_t row = (size_t)y * dm.W1;
    int cost2 = 0x7fffffff, d2 = -1;
    for (int d = 0; d < dm.D; ++d) {                 // ascending x = x2 + d; "<=" keeps the largest x among equal costs
        const int xv = x2 + d - dm.D;
        if (xv >= 0 && xv < dm.W1 && best_d[row + xv] == d) {
            const int c = min_s[row + xv];
            if (c <= cost2) { cost2 = c; d2 = d; }
        }
    }
    disp2[t] = (int16_t)d2;
}

// ---- left-right check, median, depth (steps 6, 7, 8) -------------------------------------------------------------------------
__device__ __forceinline__ bool st_mismatch(const int16_t* __restrict__ d2row, int W, int x2, int d, int max_diff) {
    if (x2 < 0 || x2 >= W) return false;
    const int v = d2row[x2];
    return v >= 0 && abs(v - d) > max_diff;
}

__device__ __forceinline__ int st_checked(const int16_t* __restrict__ d16, const int16_t* __restrict__ disp2, const StereoDims& dm,
                                          int x, int y, int max_diff) {
    if (x < dm.D) return -16;
    const int v = d16[(size_t)y * dm.W1 + (x - dm.D)];
    if (v < 0) return -16;
    const int a = v >> 4, b = (v + 15) >> 4;
    const int16_t* d2row = disp2 + (size_t)y * dm.W;
    return st_mismatch(d2row, dm.W, x - a, a, max_diff) && st_mismatch(d2row, dm.W, x - b, b, max_diff) ? -16 : v;
}

__device__ __forceinline__ void st_sort2(int& a, int& b) { const int lo = min(a, b); b = max(a, b); a = lo; }

__global__ void __launch_bounds__(ST_THREADS) stereo_finish_kernel(const int16_t* __restrict__ d16, const int16_t* __restrict__ disp2,
                                                                   StereoDims dm, int max_diff, double bf,
                                                                   int16_t* __restrict__ disp16_out, float* __restrict__ depth_out) {
    const size_t t = (size_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (t >= (size_t)dm.W * dm.H) return;
    const int y = (int)(t / dm.W), x = (int)(t % dm.W);
    int v[9];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i)
            v[3 * j + i] = st_checked(d16, disp2, dm, min(max(x + i - 1, 0), dm.W - 1), min(max(y + j - 1, 0), dm.H - 1), max_diff);
    // median of nine: the 19-exchange network
    st_sort2(v[1], v[2]); st_sort2(v[4], v[5]); st_sort2(v[7], v[8]); st_sort2(v[0], v[1]); st_sort2(v[3], v[4]);
    st_sort2(v[6], v[7]); st_sort2(v[1], v[2]); st_sort2(v[4], v[5]); st_sort2(v[7], v[8]); st_sort2(v[0], v[3]);
    st_sort2(v[5], v[8]); st_sort2(v[4], v[7]); st_sort2(v[3], v[6]); st_sort2(v[1], v[4]); st_sort2(v[2], v[5]);
    st_sort2(v[4], v[7]); st_sort2(v[4], v[2]); st_sort2(v[6], v[4]); st_sort2(v[4], v[2]);
    const int m = v[4];
    disp16_out[t] = (int16_t)m;
    double disp = (double)m / 16.0;
    if (disp == 0.0) disp = 1e10;
    const double z = bf / disp;
    depth_out[t] = (float)(z < 0.0 ? 0.0 : z);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct StereoScratch {
    uint8_t *rect_l, *rect_r;         // [H][W]
    uint2 *trip_l, *trip_r;           // [H][W]
    uint32_t* cost;                   // [H][W1][D]
    uint32_t* sum;                    // [H][W1][D]; its first half holds the uint16 row sums until the first path kernel runs
    int32_t* min_s;                   // [H][W1]
    int16_t* best_d;                  // [H][W1]
    int16_t* d16;                     // [H][W1]
    int16_t* disp2;                   // [H][W]
    size_t bytes;
};

static StereoScratch st_carve(void* base, int W, int H, int D) {
    const size_t HW = (size_t)W * H, HW1 = (size_t)(W - D) * H, vol = HW1 * D;
    StereoScratch s;
    ScratchCursor c(base);
    s.rect_l = c.take<uint8_t>(HW); s.rect_r = c.take<uint8_t>(HW);
    s.trip_l = c.take<uint2>(HW * sizeof(uint2)); s.trip_r = c.take<uint2>(HW * sizeof(uint2));
    s.cost = c.take<uint32_t>(vol * sizeof(uint32_t));
    s.sum = c.take<uint32_t>(vol * sizeof(uint32_t));
    s.min_s = c.take<int32_t>(HW1 * sizeof(int32_t));
    s.best_d = c.take<int16_t>(HW1 * sizeof(int16_t));
    s.d16 = c.take<int16_t>(HW1 * sizeof(int16_t));
    s.disp2 = c.take<int16_t>(HW * sizeof(int16_t));
    s.bytes = c.used();
    return s;
}

static bool st_sizes_ok(int32_t W, int32_t H, int32_t D) {
    return D >= 16 && D <= 64 && D % 16 == 0 && H >= 1 && W > D && (size_t)(W - D) * H * D < ((size_t)1 << 31);
}

static unsigned st_blocks(size_t items, size_t per_block = ST_THREADS) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_stereo_scratch_bytes(int32_t width, int32_t height, int32_t num_disparities) {
    if (!st_sizes_ok(width, height, num_disparities)) return 256;
    size_t bytes = 0;                                  // (W - D) D is not monotone in D: the largest need up to this D
    for (int d = 16; d <= num_disparities; d += 16)
        if (width > d) bytes = std::max(bytes, st_carve(nullptr, width, height, d).bytes);
    return bytes + 256;                                // (the carve starts at the next multiple of 256)
}

int mgs_stereo_depth(const MgsStereo* p, void* stream) {
    if (!p) { set_error("mgs_stereo_depth: params must be non-NULL"); return 1; }
    const int D = p->num_disparities;
    if (D < 16 || D > 64 || D % 16 != 0) { set_error("mgs_stereo_depth: num_disparities must be 16, 32, 48 or 64 (got %d)", D); return 1; }
    if (p->height < 1 || p->width - D < 1) { set_error("mgs_stereo_depth: needs height >= 1 and width > num_disparities"); return 1; }
    if (!st_sizes_ok(p->width, p->height, D)) { set_error("mgs_stereo_depth: (width - num_disparities) x height x num_disparities must stay below 2^31"); return 1; }
    // OpenCV's parameter defaulting
    const int block = p->block_size > 0 ? p->block_size : 5;
    const int s = block / 2;
    const int P1 = p->p1 > 0 ? p->p1 : 2;
    const int P2 = max(p->p2 > 0 ? p->p2 : 5, P1 + 1);
    const int uniq = p->uniqueness_ratio >= 0 ? p->uniqueness_ratio : 10;
    const int max_diff = p->disp12_max_diff > 0 ? p->disp12_max_diff : 1;
    const int ftzero = max(p->pre_filter_cap, 15) | 1;
    if (2 * s + 1 > 63) { set_error("mgs_stereo_depth: block_size must stay below 64 (the row sums are 16-bit)"); return 1; }
    if (P1 > (1 << 20) || P2 > (1 << 20)) { set_error("mgs_stereo_depth: p1 and p2 must not exceed 2^20"); return 1; }
    if (uniq > 100) { set_error("mgs_stereo_depth: uniqueness_ratio must not exceed 100"); return 1; }
    if (ftzero > 127) { set_error("mgs_stereo_depth: pre_filter_cap must not exceed 127 (the filtered image is 8-bit)"); return 1; }
    if (!(p->bf == p->bf) || fabs(p->bf) == (double)INFINITY) { set_error("mgs_stereo_depth: bf must be finite"); return 1; }
    if (!p->left_u8 || !p->right_u8 || !p->rgb_out || !p->disp16_out || !p->depth_out || !p->scratch) {
        set_error("mgs_stereo_depth: left_u8, right_u8, rgb_out, disp16_out, depth_out and scratch must be non-NULL");
        return 1;
    }
    const int n_maps = (p->map_lx != nullptr) + (p->map_ly != nullptr) + (p->map_rx != nullptr) + (p->map_ry != nullptr);
    if (n_maps != 0 && n_maps != 4) { set_error("mgs_stereo_depth: the four rectification maps go together: all or none"); return 1; }
    if ((size_t)p->scratch % 16 != 0) { set_error("mgs_stereo_depth: scratch must be 16-byte aligned"); return 1; }
    if (p->sum_out && (size_t)p->sum_out % 4 != 0) { set_error("mgs_stereo_depth: sum_out must be 4-byte aligned"); return 1; }

    hipStream_t st = (hipStream_t)stream;
    const StereoDims dm{p->width, p->height, D, p->width - D};
    StereoScratch sc = st_carve(p->scratch, dm.W, dm.H, D);
    const size_t HW = (size_t)dm.W * dm.H, HW1 = (size_t)dm.W1 * dm.H;
    const dim3 block256(ST_THREADS);

    StereoPrepareArgs a;
    a.left = p->left_u8; a.right = p->right_u8;
    a.map_lx = p->map_lx; a.map_ly = p->map_ly; a.map_rx = p->map_rx; a.map_ry = p->map_ry;
    a.rect_l = p->left_rect_out ? p->left_rect_out : sc.rect_l;
    a.rect_r = p->right_rect_out ? p->right_rect_out : sc.rect_r;
    a.rgb_out = p->rgb_out; a.W = dm.W; a.H = dm.H;
    if (n_maps) hipLaunchKernelGGL(stereo_prepare_kernel<true>, dim3(st_blocks(HW)), block256, 0, st, a);
    else hipLaunchKernelGGL(stereo_prepare_kernel<false>, dim3(st_blocks(HW)), block256, 0, st, a);
    hipLaunchKernelGGL(stereo_prefilter_kernel, dim3(st_blocks(HW)), block256, 0, st, a.rect_l, a.rect_r, dm.W, dm.H, ftzero,
                       sc.trip_l, sc.trip_r);

    uint16_t* hs = (uint16_t*)sc.sum;
    const int xc = (dm.W1 + ST_CHUNK - 1) / ST_CHUNK, yc = (dm.H + ST_CHUNK - 1) / ST_CHUNK;
    hipLaunchKernelGGL(stereo_hsum_kernel, dim3(st_blocks((size_t)dm.H * xc * D)), block256, 0, st, sc.trip_l, sc.trip_r, dm, s, xc, hs);
    hipLaunchKernelGGL(stereo_vsum_kernel, dim3(st_blocks((size_t)dm.W1 * D * yc)), block256, 0, st, hs, dm, s, yc, sc.cost);

    uint32_t* sum = p->sum_out ? (uint32_t*)p->sum_out : sc.sum;
    const int diag = dm.W1 + dm.H - 1;
    const unsigned wpb = ST_THREADS / 64;
    hipLaunchKernelGGL((stereo_path_kernel<0, false>), dim3(st_blocks(dm.H, wpb)), block256, 0, st, sc.cost, sum, dm, (uint32_t)P1, (uint32_t)P2, dm.H);
    hipLaunchKernelGGL((stereo_path_kernel<1, true>), dim3(st_blocks(diag, wpb)), block256, 0, st, sc.cost, sum, dm, (uint32_t)P1, (uint32_t)P2, diag);
    hipLaunchKernelGGL((stereo_path_kernel<2, true>), dim3(st_blocks(dm.W1, wpb)), block256, 0, st, sc.cost, sum, dm, (uint32_t)P1, (uint32_t)P2, dm.W1);
    hipLaunchKernelGGL((stereo_path_kernel<3, true>), dim3(st_blocks(diag, wpb)), block256, 0, st, sc.cost, sum, dm, (uint32_t)P1, (uint32_t)P2, diag);
    hipLaunchKernelGGL((stereo_path_kernel<4, true>), dim3(st_blocks(dm.H, wpb)), block256, 0, st, sc.cost, sum, dm, (uint32_t)P1, (uint32_t)P2, dm.H);

    hipLaunchKernelGGL(stereo_winner_kernel, dim3(st_blocks(HW1, wpb)), block256, 0, st, sum, dm, uniq, HW1, sc.min_s, sc.best_d, sc.d16);
    hipLaunchKernelGGL(stereo_table_kernel, dim3(st_blocks(HW)), block256, 0, st, sc.min_s, sc.best_d, dm, sc.disp2);
    hipLaunchKernelGGL(stereo_finish_kernel, dim3(st_blocks(HW)), block256, 0, st, sc.d16, sc.disp2, dm, max_diff, p->bf,
                       p->disp16_out, p->depth_out);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
