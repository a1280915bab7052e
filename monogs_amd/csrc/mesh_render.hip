// Triangle-mesh rendering ("Mesh rendering"; tests/mesh_render_mirror.py restates it in float64): depth, triangle id,
// vertex colour and face label of an indexed mesh seen by a pinhole camera.  Kernels, launcher and entry points; what the Depth L1
// of metrics.hip compares.  No counterpart in the reference, which has no mesh.
//
//   clear    the key image to all ones
//   setup    one lane per triangle: index check, transform, the three canonical edge vectors and the z's as ONE 64-byte record,
//            the padded box of 8x8 pixel blocks the triangle can touch, the number of those blocks; a triangle whose padded pixel
//            box is at most 6 x 6 is rasterised right here by its lane and counts no block (MGS_MESH_NO_SMALL, a test flag,
//            sends it through the raster pass instead: the image is bit-identical)
//   scan     of the block counts, 64-bit (T <= 2^30 triangles of up to 2048 x 2048 blocks each)
//   raster   a persistent grid; a wave takes 64 consecutive (triangle, block) items, each lane finds its own by binary search in
//            the scan, then the wave walks the 64 items, one block per step, one lane per pixel; a hit whose key
//            bits(z) << 32 | triangle is below the pixel's current one issues one 64-bit atomicMin (global_atomic_umin_x2)
//   resolve  one lane per pixel: depth = the key's high word, the weights of the winner recomputed for the colour
//
// The test is projective, w_i = d . (v_j x v_k) with d the pixel's ray: a triangle with vertices behind the camera needs no
// clipping; only its box is taken from the part in front of `near`.  WATERTIGHT: v_j x v_k is formed from the two endpoints in ascending vertex-index order
// (without contraction, so that a repeated vertex gives exactly 0) and then negated when the triangle travels the edge the other
// way; w_i is one fixed fma chain, whose result negates exactly with its inputs.  Two triangles that share an edge by index see the
// same magnitude, so a ray cannot pass between them.  The image is the minimum of the keys over all hits: independent of the order
// of execution and of the triangles, bitwise reproducible.  No host synchronisation, no read-back, kernel nodes only.
#include "common.h"

namespace mgs {

constexpr int MR_THREADS = 256;
constexpr int MR_SCAN_SHIFT = 11;
constexpr int MR_SCAN_ITEMS = 1 << MR_SCAN_SHIFT;       // per scan block: 256 threads x 8 consecutive triangles
constexpr int MR_SCANB_THREADS = 1024;
constexpr int MR_BLOCK_SHIFT = 3;                       // 8x8 pixel blocks: one wave, one lane per pixel
constexpr int MR_RASTER_GROUPS = 1024;                  // the persistent grid: 256 CUs x 4 workgroups of 4 waves
constexpr int MR_SMALL = 6;                             // a padded box of at most 6 x 6 pixels is rasterised by the setup lane
constexpr int MR_REC_FLOATS = 16;                       // {e0, z0}, {e1, z1}, {e2, z2}, {block origin, block counts, -, -}
constexpr unsigned long long MR_EMPTY = ~0ull;

struct MeshRenderArgs {
    int V, T, W, H;
    const float* vert;
    const int32_t* tri;
    const float* colors;          // [V,3] or NULL
    const int32_t* face_labels;   // [T] or NULL
    const float* view;
    float fx, fy, cx, cy, near, far;
    int one_sided, fuse_small;
    float bg0, bg1, bg2;
    float* rec;                   // [T][16]
    uint64_t* incl;               // [ceil(T / 2048) * 2048] block counts, then their block-local inclusive scan
    uint64_t* blk;                // [ceil(T / 2048)] exclusive scan of the scan blocks' totals
    uint64_t* total;              // [1]
    unsigned long long* keys;     // [H][W]
    float* depth;
    int32_t* tri_id;
    float* rgb;
    int32_t* label;
    uint32_t* status;
};

// the ray of pixel (px, py): ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, 1)
__device__ __forceinline__ void mr_ray(const MeshRenderArgs& a, int px, int py, float& dx, float& dy) {
    dx = ((float)px + 0.5f - a.cx) / a.fx;
    dy = ((float)py + 0.5f - a.cy) / a.fy;
}
// w = d . e as ONE fma chain: negating e negates w exactly
__device__ __forceinline__ float mr_weight(float dx, float dy, float ex, float ey, float ez) {
    return fmaf(dx, ex, fmaf(dy, ey, ez));
}
// the edge vector a x b of the edge travelled from vertex ia to vertex ib: the cross product of the endpoint with the smaller
// index and the one with the larger, then the sign of the direction of travel
__device__ __forceinline__ void mr_edge(int ia, int ib, float ax, float ay, float az, float bx, float by, float bz, float& ex,
                                        float& ey, float& ez) {
#pragma clang fp contract(off)
    const bool swap = ia > ib;
    const float lx = swap ? bx : ax, ly = swap ? by : ay, lz = swap ? bz : az;
    const float hx = swap ? ax : bx, hy = swap ? ay : by, hz = swap ? az : bz;
    const float cx = ly * hz - lz * hy, cy = lz * hx - lx * hz, cz = lx * hy - ly * hx;
    const bool same = ia == ib;
    ex = same ? 0.f : (swap ? -cx : cx);
    ey = same ? 0.f : (swap ? -cy : cy);
    ez = same ? 0.f : (swap ? -cz : cz);
}
// hit test and depth of one ray against one record; false: no accepted hit
__device__ __forceinline__ bool mr_hit(const MeshRenderArgs& a, float w0, float w1, float w2, float z0, float z1, float z2,
                                       float& z) {
    const float S = (w0 + w1) + w2;
    const bool pos = w0 >= 0.f && w1 >= 0.f && w2 >= 0.f, neg = w0 <= 0.f && w1 <= 0.f && w2 <= 0.f;
    if (!(S != 0.f) || !(pos || neg) || (a.one_sided && !(S < 0.f))) return false;
    z = fmaf(w0, z0, fmaf(w1, z1, w2 * z2)) / S;
    return z >= a.near && (a.far <= 0.f || z <= a.far);
}

__global__ void __launch_bounds__(MR_THREADS) mesh_render_clear_kernel(unsigned long long* __restrict__ keys, size_t n) {
    for (size_t i = (size_t)blockIdx.x * MR_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * MR_THREADS) keys[i] = MR_EMPTY;
}

__global__ void __launch_bounds__(MR_THREADS) mesh_render_setup_kernel(const MeshRenderArgs a) {
    const int t = blockIdx.x * MR_THREADS + threadIdx.x;
    if (t >= a.T) return;
    const int i0 = a.tri[3 * (size_t)t], i1 = a.tri[3 * (size_t)t + 1], i2 = a.tri[3 * (size_t)t + 2];
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, r3 = r0;
    uint64_t n = 0ull;
    if ((unsigned)i0 >= (unsigned)a.V || (unsigned)i1 >= (unsigned)a.V || (unsigned)i2 >= (unsigned)a.V) {
        atomicOr(a.status, 1u);                                     // an argument error: nothing is read through the index
    } else {
        const ViewRows cam(MGS_CONST(a.view));
        const float p0x = a.vert[3 * (size_t)i0], p0y = a.vert[3 * (size_t)i0 + 1], p0z = a.vert[3 * (size_t)i0 + 2];
        const float p1x = a.vert[3 * (size_t)i1], p1y = a.vert[3 * (size_t)i1 + 1], p1z = a.vert[3 * (size_t)i1 + 2];
        const float p2x = a.vert[3 * (size_t)i2], p2y = a.vert[3 * (size_t)i2 + 1], p2z = a.vert[3 * (size_t)i2 + 2];
        MGS_TO_CAMERA(cam, p0x, p0y, p0z, x0, y0, z0);
        MGS_TO_CAMERA(cam, p1x, p1y, p1z, x1, y1, z1);
        MGS_TO_CAMERA(cam, p2x, p2y, p2z, x2, y2, z2);
        mr_edge(i1, i2, x1, y1, z1, x2, y2, z2, r0.x, r0.y, r0.z);   // w0 = d . (v1 x v2)
        mr_edge(i2, i0, x2, y2, z2, x0, y0, z0, r1.x, r1.y, r1.z);   // w1 = d . (v2 x v0)
        mr_edge(i0, i1, x0, y0, z0, x1, y1, z1, r2.x, r2.y, r2.z);   // w2 = d . (v0 x v1)
        r0.w = z0; r1.w = z1; r2.w = z2;
        // The pixels the triangle can own.  A hit's depth is a convex combination of the three z's: nothing nearer than `near`
        // or beyond `far` as a whole is kept, and an accepted hit lies on the part of the triangle at z >= near.  That part is
        // a convex polygon -- the vertices in front and, on each edge that crosses, the point at zc = 0.999 near -- and its image
        // lies inside the box of the projections of those points, padded by a pixel (their rounding is far below that: the
        // coordinates are clamped to the image first).  A projection that is no number: the whole image.
        const float zmin = fminf(z0, fminf(z1, z2)), zmax = fmaxf(z0, fmaxf(z1, z2));
        bool live = zmax >= a.near * 0.9999f && !(a.far > 0.f && zmin > a.far * 1.0001f);     // (margins: the rounding of a hit's z)
        float bx0 = 0.f, by0 = 0.f, bx1 = (float)(a.W - 1), by1 = (float)(a.H - 1);
        if (live) {
            const float zc = a.near * 0.999f, inf = __int_as_float(0x7f800000);
            float lo_u = inf, hi_u = -inf, lo_v = inf, hi_v = -inf;
            bool bad = false;
            auto add = [&](float x, float y, float z) {
                const float u = a.fx * x / z + a.cx - 0.5f, v = a.fy * y / z + a.cy - 0.5f;
                bad |= (u != u) || (v != v);
                lo_u = fminf(lo_u, u); hi_u = fmaxf(hi_u, u); lo_v = fminf(lo_v, v); hi_v = fmaxf(hi_v, v);
            };
            auto corner = [&](float xa, float ya, float za, float xb, float yb, float zb) {      // vertex a, and edge a -> b
                if (za >= zc) add(xa, ya, za);
                if ((za >= zc) != (zb >= zc)) {
                    const float s = (zc - za) / (zb - za);
                    add(xa + s * (xb - xa), ya + s * (yb - ya), zc);
                }
            };
            corner(x0, y0, z0, x1, y1, z1);
            corner(x1, y1, z1, x2, y2, z2);
            corner(x2, y2, z2, x0, y0, z0);
            if (!bad) {
                lo_u = floorf(lo_u) - 1.f; hi_u = ceilf(hi_u) + 1.f; lo_v = floorf(lo_v) - 1.f; hi_v = ceilf(hi_v) + 1.f;
                live = lo_u <= bx1 && hi_u >= 0.f && lo_v <= by1 && hi_v >= 0.f;
                bx0 = fmaxf(lo_u, 0.f); bx1 = fminf(hi_u, bx1);
                by0 = fmaxf(lo_v, 0.f); by1 = fminf(hi_v, by1);
            }
        }
        // A triangle whose padded box is at most 6 x 6 pixels (scan density: most of a fine mesh) is finished here, by its own lane:
        // the same ray, weights, test and key as the raster pass, at most 36 pixels, and no (triangle, block) item at all.
        if (live && a.fuse_small && bx1 - bx0 < (float)MR_SMALL && by1 - by0 < (float)MR_SMALL) {
            for (int py = (int)by0; py <= (int)by1; ++py)
                for (int px = (int)bx0; px <= (int)bx1; ++px) {
                    float dx, dy, z;
                    mr_ray(a, px, py, dx, dy);
                    const float w0 = mr_weight(dx, dy, r0.x, r0.y, r0.z), w1 = mr_weight(dx, dy, r1.x, r1.y, r1.z),
                                w2 = mr_weight(dx, dy, r2.x, r2.y, r2.z);
                    if (mr_hit(a, w0, w1, w2, z0, z1, z2, z)) {
                        const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (uint32_t)t;
                        unsigned long long* p = a.keys + (size_t)py * a.W + px;
                        if (key < __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMin(p, key);
                    }
                }
            live = false;
        }
        if (live) {
            const uint32_t cx0 = (uint32_t)(int)bx0 >> MR_BLOCK_SHIFT, cx1 = (uint32_t)(int)bx1 >> MR_BLOCK_SHIFT;
            const uint32_t cy0 = (uint32_t)(int)by0 >> MR_BLOCK_SHIFT, cy1 = (uint32_t)(int)by1 >> MR_BLOCK_SHIFT;
            const uint32_t nx = cx1 - cx0 + 1u, ny = cy1 - cy0 + 1u;                 // <= 2048 each: images stay within 16384
            r3.x = __uint_as_float(cx0 | (cy0 << 16));
            r3.y = __uint_as_float(nx | (ny << 16));
            n = (uint64_t)nx * ny;
        }
    }
    float4* rec = (float4*)a.rec + 4 * (size_t)t;
    rec[0] = r0; rec[1] = r1; rec[2] = r2; rec[3] = r3;
    a.incl[t] = n;
}

// block-local inclusive scan in place; a thread owns 8 consecutive items, items at index >= T count as 0
__global__ void __launch_bounds__(MR_THREADS) mesh_render_scan_local_kernel(uint64_t* __restrict__ incl, uint64_t* __restrict__ blk, int T) {
    __shared__ uint64_t s_w[MR_THREADS / WAVE];
    const size_t base = (size_t)blockIdx.x * MR_SCAN_ITEMS + (size_t)threadIdx.x * 8;
    uint64_t x[8], sum = 0ull;
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        sum += base + n < (size_t)T ? incl[base + n] : 0ull;
        x[n] = sum;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t in = wave_incl_scan_u64(sum, lane);
    if (lane == 63) s_w[wv] = in;
    __syncthreads();
    uint64_t before = in - sum, total = 0ull;
#pragma unroll
    for (int w = 0; w < MR_THREADS / WAVE; ++w) {
        before += w < wv ? s_w[w] : 0ull;
        total += s_w[w];
    }
#pragma unroll
    for (int n = 0; n < 8; ++n) incl[base + n] = x[n] + before;      // (the scratch holds whole scan blocks)
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the block sums in place, and the grand total (nb == 0: the total is 0)
__global__ void __launch_bounds__(MR_SCANB_THREADS) mesh_render_scan_blocks_kernel(uint64_t* __restrict__ blk, uint32_t nb,
                                                                                   uint64_t* __restrict__ total_out) {
    __shared__ uint64_t s_w[MR_SCANB_THREADS / WAVE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t carry = 0ull;
    for (uint32_t b0 = 0; b0 < nb; b0 += MR_SCANB_THREADS) {
        const uint32_t b = b0 + threadIdx.x;
        const uint64_t x = b < nb ? blk[b] : 0ull;
        const uint64_t in = wave_incl_scan_u64(x, lane);
        if (lane == 63) s_w[wv] = in;
        __syncthreads();
        uint64_t before = carry, total = 0ull;
        for (int w = 0; w < MR_SCANB_THREADS / WAVE; ++w) {
            before += w < wv ? s_w[w] : 0ull;
            total += s_w[w];
        }
        before += in - x;
        if (b < nb) blk[b] = before;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) total_out[0] = carry;
}

__global__ void __launch_bounds__(MR_THREADS) mesh_render_raster_kernel(const MeshRenderArgs a) {
    const uint64_t total = a.total[0];
    const int lane = threadIdx.x & 63;
    const int lx = lane & 7, ly = lane >> 3;
    const uint64_t step = (uint64_t)gridDim.x * (MR_THREADS / WAVE) * WAVE;
    for (uint64_t base = ((uint64_t)blockIdx.x * (MR_THREADS / WAVE) + (threadIdx.x >> 6)) * WAVE; base < total; base += step) {
        // every lane resolves its own item: the first triangle whose inclusive sum exceeds it (the last one's is total > item)
        const uint64_t item = base + lane;
        uint32_t my_t = 0u, my_b = 0u;
        if (item < total) {
            int lo = 0, hi = a.T - 1;
            while (lo < hi) {
                const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
                if (a.incl[mid] + a.blk[mid >> MR_SCAN_SHIFT] > item) hi = mid;
                else lo = mid + 1;
            }
            const uint32_t org = __float_as_uint(a.rec[(size_t)lo * MR_REC_FLOATS + 12]);
            const uint32_t cnt = __float_as_uint(a.rec[(size_t)lo * MR_REC_FLOATS + 13]);
            const uint32_t nx = cnt & 0xFFFFu, ny = cnt >> 16;
            const uint64_t first = a.incl[lo] + a.blk[lo >> MR_SCAN_SHIFT] - (uint64_t)nx * ny;
            const uint32_t j = (uint32_t)(item - first);               // < nx ny <= 2^22
            my_t = (uint32_t)lo;
            my_b = ((org & 0xFFFFu) + j % nx) | (((org >> 16) + j / nx) << 16);
        }
        const int n_items = total - base < (uint64_t)WAVE ? (int)(total - base) : WAVE;
        // the wave walks the items: one 8x8 block per step, one lane per pixel, the record through the scalar cache
        for (int i = 0; i < n_items; ++i) {
            const uint32_t t = bcast(my_t, i), b = bcast(my_b, i);
            const int px = (int)((b & 0xFFFFu) << MR_BLOCK_SHIFT) + lx, py = (int)((b >> 16) << MR_BLOCK_SHIFT) + ly;
            const_float_p r = MGS_CONST(a.rec) + (size_t)t * MR_REC_FLOATS;
            if (px < a.W && py < a.H) {
                float dx, dy, z;
                mr_ray(a, px, py, dx, dy);
                const float w0 = mr_weight(dx, dy, r[0], r[1], r[2]), w1 = mr_weight(dx, dy, r[4], r[5], r[6]),
                            w2 = mr_weight(dx, dy, r[8], r[9], r[10]);
                if (mr_hit(a, w0, w1, w2, r[3], r[7], r[11], z)) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | t;
                    unsigned long long* p = a.keys + (size_t)py * a.W + px;
                    // (an older, larger value read here only costs an atomic: the keys only ever fall)
                    if (key < __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMin(p, key);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(MR_THREADS) mesh_render_resolve_kernel(const MeshRenderArgs a) {
    const size_t HW = (size_t)a.W * a.H;
    const size_t pix = (size_t)blockIdx.x * MR_THREADS + threadIdx.x;
    if (pix >= HW) return;
    const unsigned long long key = a.keys[pix];
    const bool hit = key != MR_EMPTY;
    const uint32_t t = (uint32_t)key;
    a.depth[pix] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;     // exactly the raster pass's value
    if (a.tri_id) a.tri_id[pix] = hit ? (int32_t)t : -1;
    if (a.label) a.label[pix] = hit ? a.face_labels[t] : -1;
    if (a.rgb) {
        float c0 = a.bg0, c1 = a.bg1, c2 = a.bg2;
        if (hit) {
            const float4* rec = (const float4*)a.rec + 4 * (size_t)t;
            const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
            float dx, dy;
            mr_ray(a, (int)(pix % a.W), (int)(pix / a.W), dx, dy);
            const float w0 = mr_weight(dx, dy, r0.x, r0.y, r0.z), w1 = mr_weight(dx, dy, r1.x, r1.y, r1.z),
                        w2 = mr_weight(dx, dy, r2.x, r2.y, r2.z);
            const float S = (w0 + w1) + w2;
            const float* ca = a.colors + 3 * (size_t)a.tri[3 * (size_t)t];          // (in range: the triangle was set up)
            const float* cb = a.colors + 3 * (size_t)a.tri[3 * (size_t)t + 1];
            const float* cc = a.colors + 3 * (size_t)a.tri[3 * (size_t)t + 2];
            c0 = fmaf(w0, ca[0], fmaf(w1, cb[0], w2 * cc[0])) / S;
            c1 = fmaf(w0, ca[1], fmaf(w1, cb[1], w2 * cc[1])) / S;
            c2 = fmaf(w0, ca[2], fmaf(w1, cb[2], w2 * cc[2])) / S;
        }
        a.rgb[pix] = c0; a.rgb[HW + pix] = c1; a.rgb[2 * HW + pix] = c2;
    }
}

struct MeshRenderScratch {
    float* rec;
    uint64_t *incl, *blk, *total;
    unsigned long long* keys;
    size_t bytes;
};
static MeshRenderScratch mesh_render_carve(void* base, int T, int W, int H) {
    const size_t nb = ((size_t)T + MR_SCAN_ITEMS - 1) >> MR_SCAN_SHIFT;
    ScratchCursor c(base);
    MeshRenderScratch s;
    s.rec = c.take<float>((size_t)T * MR_REC_FLOATS * sizeof(float));
    s.incl = c.take<uint64_t>(nb * MR_SCAN_ITEMS * 8);
    s.blk = c.take<uint64_t>((nb + 1) * 8);
    s.total = c.take<uint64_t>(8);
    s.keys = c.take<unsigned long long>((size_t)W * H * 8);
    s.bytes = c.used() + ScratchCursor::ALIGN;
    return s;
}
static bool mesh_render_sizes_ok(int32_t T, int32_t W, int32_t H) {
    return T >= 0 && T <= (1 << 30) && W >= 1 && H >= 1 && W <= MGS_MESH_RENDER_MAX_IMAGE && H <= MGS_MESH_RENDER_MAX_IMAGE;
}

}  // namespace mgs

extern "C" {

size_t mgs_mesh_render_scratch_bytes(int32_t T, int32_t W, int32_t H) {
    if (!mgs::mesh_render_sizes_ok(T, W, H)) return 256;
    return mgs::mesh_render_carve(nullptr, T, W, H).bytes;
}

int mgs_mesh_render(const MgsMeshRender* p, void* scratch, void* stream) {
    using namespace mgs;
    const char* who = "mgs_mesh_render";
    if (!p) { set_error("%s: params is NULL", who); return 1; }
    if (p->V < 0 || p->T < 0) { set_error("%s: V and T must not be negative", who); return 1; }
    if (p->V > (1 << 30) || p->T > (1 << 30)) { set_error("%s: V and T must stay within 2^30", who); return 1; }
    if (p->W < 1 || p->H < 1 || p->W > MGS_MESH_RENDER_MAX_IMAGE || p->H > MGS_MESH_RENDER_MAX_IMAGE) {
        set_error("%s: the image must be 1 .. %d pixels wide and high", who, MGS_MESH_RENDER_MAX_IMAGE);
        return 1;
    }
    if (!(p->fx > 0.f) || !(p->fy > 0.f)) { set_error("%s: fx and fy must be positive", who); return 1; }
    if (p->flags & ~(MGS_MESH_ONE_SIDED | MGS_MESH_NO_SMALL)) { set_error("%s: unknown flags", who); return 1; }
    if (!p->viewmatrix || !p->depth || !p->status || !scratch || (p->T > 0 && (!p->triangles || (p->V > 0 && !p->vertices)))) {
        set_error("%s: vertices, triangles, viewmatrix, depth, status and scratch must be non-NULL", who);
        return 1;
    }
    if (p->rgb && !p->colors) { set_error("%s: rgb wanted from a mesh without colors", who); return 1; }
    if (p->label && !p->face_labels) { set_error("%s: label wanted without face_labels", who); return 1; }
    const MeshRenderScratch sc = mesh_render_carve(scratch, p->T, p->W, p->H);
    MeshRenderArgs a;
    a.V = p->V; a.T = p->T; a.W = p->W; a.H = p->H;
    a.vert = p->vertices; a.tri = p->triangles; a.colors = p->colors; a.face_labels = p->face_labels; a.view = p->viewmatrix;
    a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy;
    a.near = p->near > 0.f ? p->near : 1.17549435e-38f;            // depths are positive: their bits order the keys
    a.far = p->far;
    a.one_sided = (p->flags & MGS_MESH_ONE_SIDED) ? 1 : 0;
    a.fuse_small = (p->flags & MGS_MESH_NO_SMALL) ? 0 : 1;
    a.bg0 = p->bg[0]; a.bg1 = p->bg[1]; a.bg2 = p->bg[2];
    a.rec = sc.rec; a.incl = sc.incl; a.blk = sc.blk; a.total = sc.total; a.keys = sc.keys;
    a.depth = p->depth; a.tri_id = p->tri_id; a.rgb = p->rgb; a.label = p->label; a.status = p->status;
    hipStream_t s = (hipStream_t)stream;
    const size_t HW = (size_t)a.W * a.H;
    const unsigned pix_blocks = (unsigned)((HW + MR_THREADS - 1) / MR_THREADS);
    hipLaunchKernelGGL(mesh_render_clear_kernel, dim3(pix_blocks < 4096u ? pix_blocks : 4096u), dim3(MR_THREADS), 0, s, a.keys, HW);
    if (a.T > 0) {
        const uint32_t nb = (uint32_t)(((size_t)a.T + MR_SCAN_ITEMS - 1) >> MR_SCAN_SHIFT);
        hipLaunchKernelGGL(mesh_render_setup_kernel, dim3((unsigned)((a.T + MR_THREADS - 1) / MR_THREADS)), dim3(MR_THREADS), 0, s, a);
        hipLaunchKernelGGL(mesh_render_scan_local_kernel, dim3(nb), dim3(MR_THREADS), 0, s, a.incl, a.blk, a.T);
        hipLaunchKernelGGL(mesh_render_scan_blocks_kernel, dim3(1), dim3(MR_SCANB_THREADS), 0, s, a.blk, nb, a.total);
        hipLaunchKernelGGL(mesh_render_raster_kernel, dim3(MR_RASTER_GROUPS), dim3(MR_THREADS), 0, s, a);
    }
    hipLaunchKernelGGL(mesh_render_resolve_kernel, dim3(pix_blocks), dim3(MR_THREADS), 0, s, a);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
