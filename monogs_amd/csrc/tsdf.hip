// TSDF fusion of depth images into a dense voxel grid, and extraction of an indexed triangle mesh from it by marching
// tetrahedra.  The specification is DESIGN.md, "TSDF fusion and mesh extraction"; tests/tsdf_mirror.py restates it in float64.
// No counterpart in the reference (it ends with a cloud of Gaussians); nothing here is ported.
//
// Grid: nx x ny x nz voxels, centre of (i, j, k) = origin + s (i, j, k), linear index (k ny + j) nx + i.  Every per-voxel
// kernel gives a WAVE 64 consecutive x of one (j, k) row ("brick"): the planes are read and written in whole lines, (j, k) are
// wave-uniform, and a voxel is owned by exactly one lane -- no atomics anywhere, results bitwise reproducible.
//
// integrate: one launch.  A wave first tests its brick's bounding sphere against the camera (behind depth_min, outside one of
// the four image planes, beyond depth_max + trunc) and leaves without touching memory; the test is conservative, so the
// result equals the unculled one bit for bit.  Surviving lanes project their voxel centre, gather one depth (and opacity,
// colour) value, and only those that pass sdf >= -trunc read and write the state planes.
//
// extract, count phase (5 launches): classify (the ONE read of tsdf / weight: a byte per voxel, bit 0 observed, bit 1 inside),
// cells (8 bytes of the halo through the cache -> valid byte + triangle count 0..12), edges (7-bit mask of the owned edges that
// carry a vertex), a block-local exclusive scan of both count planes in one launch, and one launch that scans the block sums of
// both and writes {V, T}.  Emit phase (2 launches): vertices at vbase[owner] + popcount(mask & (bit - 1)), triangles at
// tbase[cell] + local number with their indices looked up the same way.
//
// The six tetrahedra of a cell share the diagonal corner 000 -> 111: tetrahedron t walks 000 -> +a -> +a+b -> 111 for the
// t-th permutation (a, b, c) of the axes, so its six edges are all of the seven owned directions (three axis edges, three
// face diagonals, the body diagonal) leaving their LOWER end.  The 16 sign cases of one positively oriented tetrahedron are
// derived at compile time (tet_case); an odd permutation swaps two indices of each triangle.
#include "common.h"

namespace mgs {

constexpr int TS_THREADS = 256;                 // 4 waves: 4 bricks
constexpr int TS_SCAN_ITEMS = 2048;             // per scan block: 256 threads x 8 consecutive bytes
constexpr int TS_SCAN_SHIFT = 11;
constexpr int TS_SCANB_THREADS = 1024;

// ---- scratch of the extraction ------------------------------------------------------------------------------------------
struct TsdfScratch {
    uint8_t* cls;        // [Np] bit 0 observed, bit 1 inside
    uint8_t* valid;      // [Np] cell valid
    uint8_t* tcnt;       // [Np] triangles of the cell, 0..12
    uint8_t* emask;      // [Np] owned edges that carry a vertex
    uint32_t* vloc;      // [Np] exclusive scan of popcount(emask) inside the voxel's scan block
    uint32_t* tloc;      // [Np] the same of tcnt
    uint32_t* vblk;      // [nb] exclusive scan of the block sums
    uint32_t* tblk;      // [nb]
    size_t bytes;
};
// Np = N rounded up to whole scan blocks: the scans read and write whole blocks (the pad is masked by index, never trusted)
static TsdfScratch tsdf_carve(void* base, size_t N) {
    const size_t Np = align_up(N, TS_SCAN_ITEMS), nb = Np / TS_SCAN_ITEMS;
    ScratchCursor c(base);
    TsdfScratch s;
    s.cls = c.take<uint8_t>(Np);
    s.valid = c.take<uint8_t>(Np);
    s.tcnt = c.take<uint8_t>(Np);
    s.emask = c.take<uint8_t>(Np);
    s.vloc = c.take<uint32_t>(Np * 4);
    s.tloc = c.take<uint32_t>(Np * 4);
    s.vblk = c.take<uint32_t>(nb * 4);
    s.tblk = c.take<uint32_t>(nb * 4);
    s.bytes = c.used() + ScratchCursor::ALIGN;      // (read only from a sizing call, whose base is NULL: the slack of rounding the base up)
    return s;
}

struct TsdfGrid {
    int nx, ny, nz, xchunks;     // xchunks = ceil(nx / 64)
    float ox, oy, oz, s;
};

// the wave's brick: row (j, k), first x i0; false (wave-uniform) beyond the grid
__device__ __forceinline__ bool tsdf_brick(const TsdfGrid& g, int& i0, int& j, int& k) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (TS_THREADS / WAVE) + (threadIdx.x >> 6));
    const uint32_t row = wave / (uint32_t)g.xchunks;
    if (row >= (uint32_t)g.ny * (uint32_t)g.nz) return false;
    i0 = (int)(wave - row * (uint32_t)g.xchunks) * WAVE;
    k = (int)(row / (uint32_t)g.ny);
    j = (int)(row - (uint32_t)k * (uint32_t)g.ny);
    return true;
}
static unsigned tsdf_blocks(const TsdfGrid& g) {
    const size_t waves = (size_t)g.xchunks * g.ny * g.nz;
    return (unsigned)((waves + TS_THREADS / WAVE - 1) / (TS_THREADS / WAVE));
}

// ---- integrate ----------------------------------------------------------------------------------------------------------
struct TsdfIntegrateArgs {
    TsdfGrid g;
    float *tsdf, *weight, *r, *gr, *b;        // colour planes NULL: no colour
    const float *depth, *opacity, *rgb;       // opacity, rgb may be NULL
    const float* view;                        // the transposed world->camera matrix of mgs_camera.viewmatrix
    int W, H;
    float fx, fy, cx, cy, trunc, depth_min, depth_max, opacity_min, max_weight;
    int cull;
};

__global__ void __launch_bounds__(TS_THREADS) tsdf_integrate_kernel(const TsdfIntegrateArgs a) {
    int i0, j, k;
    if (!tsdf_brick(a.g, i0, j, k)) return;
    const ViewRows cam(MGS_CONST(a.view));
    const float s = a.g.s;
    const float py = a.g.oy + s * (float)j, pz = a.g.oz + s * (float)k;
    if (a.cull) {
        // bounding sphere of the brick's voxel centres: the midpoint of the run, half its length (the rotation keeps lengths),
        // widened by far more than float32 rounding of these few operations can move a point
        const int n = min(WAVE, a.g.nx - i0);
        const float half = 0.5f * s * (float)(n - 1);
        const float mx = a.g.ox + s * (float)i0 + half;
        MGS_TO_CAMERA(cam, mx, py, pz, X, Y, Z);
        const float rad = half * 1.001f + 0.01f * s + 1e-4f * (fabsf(X) + fabsf(Y) + fabsf(Z) + 1.f);
        if (Z + rad < a.depth_min) return;                                       // step 1 fails for every voxel
        if (a.depth_max > 0.f && Z - rad > a.depth_max + a.trunc) return;        // d <= depth_max: sdf < -trunc for every voxel
        if (a.depth_min >= 0.f) {
            // every voxel that passes step 1 has z > 0: pixel x in [0, W) <=> fx x + cx z >= 0 and fx x + (cx - W) z < 0
            const float cxr = a.cx - (float)a.W, cyr = a.cy - (float)a.H;
            const float ml = 1e-4f * (fabsf(a.fx * X) + fabsf(a.cx * Z)), mr = 1e-4f * (fabsf(a.fx * X) + fabsf(cxr * Z));
            const float mt = 1e-4f * (fabsf(a.fy * Y) + fabsf(a.cy * Z)), mb = 1e-4f * (fabsf(a.fy * Y) + fabsf(cyr * Z));
            if (a.fx * X + a.cx * Z < -(rad * sqrtf(a.fx * a.fx + a.cx * a.cx) + ml)) return;
            if (a.fx * X + cxr * Z > rad * sqrtf(a.fx * a.fx + cxr * cxr) + mr) return;
            if (a.fy * Y + a.cy * Z < -(rad * sqrtf(a.fy * a.fy + a.cy * a.cy) + mt)) return;
            if (a.fy * Y + cyr * Z > rad * sqrtf(a.fy * a.fy + cyr * cyr) + mb) return;
        }
    }
    const int i = i0 + (int)(threadIdx.x & 63);
    if (i >= a.g.nx) return;
    const float px = a.g.ox + s * (float)i;
    MGS_TO_CAMERA(cam, px, py, pz, x, y, z);
    if (!(z > a.depth_min)) return;                                              // 1
    size_t pix;
    if (!camera_pixel(a.fx, a.fy, a.cx, a.cy, a.W, a.H, x, y, z, pix)) return;   // 2
    float d = a.depth[pix];                                                      // 3
    if (a.opacity) {
        const float al = a.opacity[pix];
        if (!(al >= a.opacity_min)) return;
        d = d / al;
    }
    if (!(d > a.depth_min) || (a.depth_max > 0.f && d > a.depth_max)) return;
    const float sdf = d - z;                                                     // 4
    if (!(sdf >= -a.trunc)) return;
    const float f = fminf(1.f, sdf / a.trunc);
    const size_t vi = ((size_t)k * a.g.ny + j) * a.g.nx + i;                     // 5
    const float w = a.weight[vi], w1 = w + 1.f;
    a.tsdf[vi] = (a.tsdf[vi] * w + f) / w1;
    if (a.r && a.rgb) {
        const size_t HW = (size_t)a.W * a.H;
        a.r[vi] = (a.r[vi] * w + a.rgb[pix]) / w1;
        a.gr[vi] = (a.gr[vi] * w + a.rgb[HW + pix]) / w1;
        a.b[vi] = (a.b[vi] * w + a.rgb[2 * HW + pix]) / w1;
    }
    a.weight[vi] = fminf(w1, a.max_weight);
}

// ---- the tetrahedra -----------------------------------------------------------------------------------------------------
// owned edge bits: 0 +x, 1 +y, 2 +z, 3 +x+y, 4 +y+z, 5 +x+z, 6 +x+y+z
__host__ __device__ constexpr int ts_perm(int t, int n) {          // axis n of the t-th permutation, lexicographic
    constexpr int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    return P[t][n];
}
__host__ __device__ constexpr bool ts_odd(int t) { return t == 1 || t == 2 || t == 5; }
__host__ __device__ constexpr int ts_diag_bit(int a, int b) { return a + b == 1 ? 3 : (a + b == 3 ? 4 : 5); }
// corner mask (bit 0 x, bit 1 y, bit 2 z) of vertex n = 0..3 of tetrahedron t
__host__ __device__ constexpr int ts_corner(int t, int n) {
    return n == 0 ? 0 : n == 1 ? (1 << ts_perm(t, 0)) : n == 2 ? ((1 << ts_perm(t, 0)) | (1 << ts_perm(t, 1))) : 7;
}
// local edge e of tetrahedron t: 0 (v0 v1), 1 (v1 v2), 2 (v2 v3), 3 (v0 v2), 4 (v1 v3), 5 (v0 v3); its owner is the lower vertex
__host__ __device__ constexpr int ts_edge_owner(int t, int e) { return ts_corner(t, e == 1 || e == 4 ? 1 : (e == 2 ? 2 : 0)); }
__host__ __device__ constexpr int ts_edge_bit(int t, int e) {
    return e < 3 ? ts_perm(t, e) : e == 3 ? ts_diag_bit(ts_perm(t, 0), ts_perm(t, 1))
                                 : e == 4 ? ts_diag_bit(ts_perm(t, 1), ts_perm(t, 2)) : 6;
}
__host__ __device__ constexpr int ts_local_edge(int p, int q) {    // of the vertex pair p != q
    const int lo = p < q ? p : q, hi = p < q ? q : p;
    return hi - lo == 1 ? lo : (hi - lo == 2 ? 3 + lo : 5);
}
// one sign case of a POSITIVELY oriented tetrahedron (det(v1 - v0, v2 - v0, v3 - v0) > 0), bit n of m set: vertex n inside.
// Packed: triangles in bits 0..1, then local edge ids of 3 bits each.  The normal points to the outside (positive) vertices:
//   one vertex p apart from the others q0 < q1 < q2: the face (q0, q1, q2) seen from p is oriented (-1)^p;
//   two inside p < q, two outside r < s: the quad (pr, ps, qs, qr) faces the outside when (p, q, r, s) is an even permutation.
__host__ __device__ constexpr uint32_t tet_case(int m) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int n = 0; n < 4; ++n) {
        if ((m >> n) & 1) in[ni++] = n;
        else out[no++] = n;
    }
    if (ni == 0 || ni == 4) return 0u;
    int e[6] = {0, 0, 0, 0, 0, 0}, nt = 1;
    if (ni == 1 || ni == 3) {
        const int p = ni == 1 ? in[0] : out[0];
        const int* q = ni == 1 ? out : in;
        bool keep = (p & 1) == 0;
        if (ni == 3) keep = !keep;
        e[0] = ts_local_edge(p, q[0]);
        e[1] = ts_local_edge(p, keep ? q[1] : q[2]);
        e[2] = ts_local_edge(p, keep ? q[2] : q[1]);
    } else {
        const int p = in[0], q = in[1], r = out[0], s = out[1];
        const int perm[4] = {p, q, r, s};
        int inv = 0;
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j) inv += perm[i] > perm[j] ? 1 : 0;
        const int A = ts_local_edge(p, r), B = ts_local_edge(p, s), Cc = ts_local_edge(q, s), D = ts_local_edge(q, r);
        nt = 2;
        if ((inv & 1) == 0) { e[0] = A; e[1] = B; e[2] = Cc; e[3] = A; e[4] = Cc; e[5] = D; }
        else { e[0] = A; e[1] = Cc; e[2] = B; e[3] = A; e[4] = D; e[5] = Cc; }
    }
    uint32_t w = (uint32_t)nt;
    for (int i = 0; i < 6; ++i) w |= (uint32_t)e[i] << (2 + 3 * i);
    return w;
}
__constant__ const uint32_t TS_CASES[16] = {tet_case(0), tet_case(1), tet_case(2), tet_case(3), tet_case(4), tet_case(5),
                                            tet_case(6), tet_case(7), tet_case(8), tet_case(9), tet_case(10), tet_case(11),
                                            tet_case(12), tet_case(13), tet_case(14), tet_case(15)};

// inside bits of the four vertices of tetrahedron T from the cell's 8 corner bits
template <int T>
__device__ __forceinline__ uint32_t ts_tet_mask(uint32_t corners) {
    return ((corners >> ts_corner(T, 0)) & 1u) | (((corners >> ts_corner(T, 1)) & 1u) << 1) |
           (((corners >> ts_corner(T, 2)) & 1u) << 2) | (((corners >> ts_corner(T, 3)) & 1u) << 3);
}
__device__ __forceinline__ uint32_t ts_tris(uint32_t m) {          // 0, 1, 2 triangles for 0/4, 1/3, 2 vertices inside
    const uint32_t c = (uint32_t)__popc(m);
    return c == 2u ? 2u : (c & 1u);
}

// ---- count phase ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TS_THREADS) tsdf_classify_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                   float min_weight, size_t N, uint8_t* __restrict__ cls) {
    const size_t stride = (size_t)gridDim.x * TS_THREADS;
    for (size_t v = (size_t)blockIdx.x * TS_THREADS + threadIdx.x; v < N; v += stride)
        cls[v] = (uint8_t)((weight[v] >= min_weight ? 1u : 0u) | (tsdf[v] < 0.f ? 2u : 0u));
}

// the 8 class bytes of the cell at voxel index v (corner c at v + off(c)); the caller guarantees that they exist
__device__ __forceinline__ void ts_corners(const uint8_t* __restrict__ cls, size_t v, size_t sy, size_t sz, uint32_t& obs, uint32_t& ins) {
    obs = 0xffu; ins = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t b = cls[v + (c & 1) + ((c >> 1) & 1) * sy + ((c >> 2) & 1) * sz];
        obs &= (b & 1u) ? 0xffu : ~(1u << c);
        ins |= ((b >> 1) & 1u) << c;
    }
}
template <int T>
__device__ __forceinline__ uint32_t ts_count_tets(uint32_t ins) {
    if constexpr (T == 6) return 0u;
    else return ts_tris(ts_tet_mask<T>(ins)) + ts_count_tets<T + 1>(ins);
}

__global__ void __launch_bounds__(TS_THREADS) tsdf_cells_kernel(const TsdfGrid g, const uint8_t* __restrict__ cls,
                                                                uint8_t* __restrict__ valid, uint8_t* __restrict__ tcnt) {
    int i0, j, k;
    if (!tsdf_brick(g, i0, j, k)) return;
    const int i = i0 + (int)(threadIdx.x & 63);
    if (i >= g.nx) return;
    const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny, v = (size_t)k * sz + (size_t)j * sy + i;
    uint32_t ok = 0u, n = 0u;
    if (i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1) {
        uint32_t obs, ins;
        ts_corners(cls, v, sy, sz, obs, ins);
        ok = obs == 0xffu ? 1u : 0u;
        n = ok ? ts_count_tets<0>(ins) : 0u;
    }
    valid[v] = (uint8_t)ok;
    tcnt[v] = (uint8_t)n;
}

__global__ void __launch_bounds__(TS_THREADS) tsdf_edges_kernel(const TsdfGrid g, const uint8_t* __restrict__ cls,
                                                                const uint8_t* __restrict__ valid, uint8_t* __restrict__ emask) {
    int i0, j, k;
    if (!tsdf_brick(g, i0, j, k)) return;
    const int i = i0 + (int)(threadIdx.x & 63);
    if (i >= g.nx) return;
    const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny, v = (size_t)k * sz + (size_t)j * sy + i;
    // valid bytes of the 8 cells with base v - (a, b, c), a, b, c in {0, 1}: bit a | b << 1 | c << 2 (cells past the upper
    // faces were written 0 by tsdf_cells_kernel; the ones below index 0 do not exist)
    uint32_t cells = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int a = c & 1, b = (c >> 1) & 1, d = (c >> 2) & 1;
        if (i - a >= 0 && j - b >= 0 && k - d >= 0) cells |= (valid[v - a - b * sy - d * sz] ? 1u : 0u) << c;
    }
    const uint32_t in_a = (cls[v] >> 1) & 1u;
    uint32_t mask = 0u;
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        constexpr int DX[7] = {1, 0, 0, 1, 0, 1, 1}, DY[7] = {0, 1, 0, 1, 1, 0, 1}, DZ[7] = {0, 0, 1, 0, 1, 1, 1};
        const int dx = DX[e], dy = DY[e], dz = DZ[e];
        if (i + dx >= g.nx || j + dy >= g.ny || k + dz >= g.nz) continue;
        // the cells that contain the edge: base = v along the edge's axes, v - 1 or v along the others
        uint32_t want = 0u;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (!((c & 1) && dx) && !(((c >> 1) & 1) && dy) && !(((c >> 2) & 1) && dz)) want |= 1u << c;
        if (!(cells & want)) continue;
        const uint32_t in_b = (cls[v + dx + dy * sy + dz * sz] >> 1) & 1u;
        mask |= (in_a != in_b ? 1u : 0u) << e;
    }
    emask[v] = (uint8_t)mask;
}

// block-local exclusive scan of a byte plane (blockIdx.y = 0: popcount of emask -> vloc, 1: tcnt -> tloc) + the block's sum.
// A thread owns 8 consecutive bytes (one 8-byte load, two 16-byte stores); bytes at index >= N count as 0.
__global__ void __launch_bounds__(TS_THREADS) tsdf_scan_local_kernel(const uint8_t* __restrict__ emask, const uint8_t* __restrict__ tcnt,
                                                                     uint32_t* __restrict__ vloc, uint32_t* __restrict__ tloc,
                                                                     uint32_t* __restrict__ vblk, uint32_t* __restrict__ tblk, size_t N) {
    __shared__ uint32_t s_w[TS_THREADS / WAVE];
    const bool tri = blockIdx.y != 0;
    const uint8_t* __restrict__ src = tri ? tcnt : emask;
    uint32_t* __restrict__ dst = tri ? tloc : vloc;
    const size_t base = (size_t)blockIdx.x * TS_SCAN_ITEMS + (size_t)threadIdx.x * 8;
    const uint2 raw = *(const uint2*)(src + base);
    uint32_t x[8], sum = 0u;
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        const uint32_t b = ((n < 4 ? raw.x : raw.y) >> (8 * (n & 3))) & 255u;
        const uint32_t c = base + n < N ? (tri ? b : (uint32_t)__popc(b & 127u)) : 0u;
        x[n] = sum;
        sum += c;
    }
    const uint32_t incl = wave_incl_scan_dpp(sum);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    uint32_t before = incl - sum, total = 0u;
#pragma unroll
    for (int w = 0; w < TS_THREADS / WAVE; ++w) {
        before += w < wv ? s_w[w] : 0u;
        total += s_w[w];
    }
    uint4* o = (uint4*)(dst + base);
    o[0] = make_uint4(x[0] + before, x[1] + before, x[2] + before, x[3] + before);
    o[1] = make_uint4(x[4] + before, x[5] + before, x[6] + before, x[7] + before);
    if (threadIdx.x == 0) (tri ? tblk : vblk)[blockIdx.x] = total;
}

// one workgroup per plane: exclusive scan of the block sums in place, the grand total (saturated) to counts[plane]
__global__ void __launch_bounds__(TS_SCANB_THREADS) tsdf_scan_blocks_kernel(uint32_t* vblk, uint32_t* tblk, uint32_t nb,
                                                                            uint32_t* __restrict__ counts) {
    __shared__ unsigned long long s_w[TS_SCANB_THREADS / WAVE];
    uint32_t* blk = blockIdx.x ? tblk : vblk;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long carry = 0ull;
    for (uint32_t b0 = 0; b0 < nb; b0 += TS_SCANB_THREADS) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t x = b < nb ? blk[b] : 0u;
        const uint32_t incl = wave_incl_scan_dpp(x);          // a wave's 64 block sums: <= 64 x 2048 x 12, far below 2^32
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        unsigned long long before = carry, total = 0ull;
        for (int w = 0; w < TS_SCANB_THREADS / WAVE; ++w) {
            before += w < wv ? s_w[w] : 0ull;
            total += s_w[w];
        }
        before += incl - x;
        if (b < nb) blk[b] = (uint32_t)(before > 0xffffffffull ? 0xffffffffull : before);
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = (uint32_t)(carry > 0xffffffffull ? 0xffffffffull : carry);
}

// ---- emit phase -----------------------------------------------------------------------------------------------------------
struct TsdfEmitArgs {
    TsdfGrid g;
    const float *tsdf, *r, *gr, *b;
    const uint8_t *cls, *emask, *tcnt;
    const uint32_t *vloc, *tloc, *vblk, *tblk;
    float *vertices, *colors;
    int32_t* triangles;
    uint32_t V, T;
};

__global__ void __launch_bounds__(TS_THREADS) tsdf_emit_vertices_kernel(const TsdfEmitArgs a) {
    int i0, j, k;
    if (!tsdf_brick(a.g, i0, j, k)) return;
    const int i = i0 + (int)(threadIdx.x & 63);
    if (i >= a.g.nx) return;
    const size_t sy = (size_t)a.g.nx, sz = (size_t)a.g.nx * a.g.ny, v = (size_t)k * sz + (size_t)j * sy + i;
    const uint32_t mask = a.emask[v] & 127u;
    if (!mask) return;
    uint32_t at = a.vloc[v] + a.vblk[v >> TS_SCAN_SHIFT];
    const float s = a.g.s;
    const float pax = a.g.ox + s * (float)i, pay = a.g.oy + s * (float)j, paz = a.g.oz + s * (float)k;
    const float fa = a.tsdf[v];
    const bool col = a.colors != nullptr;
    float ra = 0.f, ga = 0.f, ba = 0.f;
    if (col) { ra = a.r[v]; ga = a.gr[v]; ba = a.b[v]; }
#pragma unroll
    for (int e = 0; e < 7; ++e) {
        constexpr int DX[7] = {1, 0, 0, 1, 0, 1, 1}, DY[7] = {0, 1, 0, 1, 1, 0, 1}, DZ[7] = {0, 0, 1, 0, 1, 1, 1};
        if (!((mask >> e) & 1u) || i + DX[e] >= a.g.nx || j + DY[e] >= a.g.ny || k + DZ[e] >= a.g.nz) continue;
        const size_t vb = v + DX[e] + DY[e] * sy + DZ[e] * sz;          // (tsdf_edges_kernel sets a bit only for an edge inside the grid)
        const float fb = a.tsdf[vb];
        const float t = fa / (fa - fb);
        if (at < a.V) {
            a.vertices[(size_t)at * 3 + 0] = pax + t * (s * (float)DX[e]);
            a.vertices[(size_t)at * 3 + 1] = pay + t * (s * (float)DY[e]);
            a.vertices[(size_t)at * 3 + 2] = paz + t * (s * (float)DZ[e]);
            if (col) {
                a.colors[(size_t)at * 3 + 0] = ra + t * (a.r[vb] - ra);
                a.colors[(size_t)at * 3 + 1] = ga + t * (a.gr[vb] - ga);
                a.colors[(size_t)at * 3 + 2] = ba + t * (a.b[vb] - ba);
            }
        }
        ++at;
    }
}

// index of the vertex on local edge E of tetrahedron T of the cell at v
template <int T>
__device__ __forceinline__ int32_t ts_vertex_index(const TsdfEmitArgs& a, size_t v, size_t sy, size_t sz, uint32_t e) {
    // the owner corner and the bit of the six local edges, chosen by the runtime edge id
    uint32_t corner = 0u, bit = 0u;
#pragma unroll
    for (int q = 0; q < 6; ++q)
        if (e == (uint32_t)q) { corner = (uint32_t)ts_edge_owner(T, q); bit = (uint32_t)ts_edge_bit(T, q); }
    const size_t o = v + (corner & 1u) + ((corner >> 1) & 1u) * sy + ((corner >> 2) & 1u) * sz;
    return (int32_t)(a.vloc[o] + a.vblk[o >> TS_SCAN_SHIFT] + (uint32_t)__popc(a.emask[o] & ((1u << bit) - 1u)));
}
template <int T>
__device__ __forceinline__ void ts_emit_tets(const TsdfEmitArgs& a, size_t v, size_t sy, size_t sz, uint32_t ins, uint32_t& at) {
    if constexpr (T < 6) {
        const uint32_t w = TS_CASES[ts_tet_mask<T>(ins)];
        const uint32_t nt = w & 3u;
        for (uint32_t n = 0; n < nt; ++n) {
            const uint32_t e0 = (w >> (2 + 9 * n)) & 7u, e1 = (w >> (5 + 9 * n)) & 7u, e2 = (w >> (8 + 9 * n)) & 7u;
            const int32_t i0 = ts_vertex_index<T>(a, v, sy, sz, e0);
            const int32_t i1 = ts_vertex_index<T>(a, v, sy, sz, ts_odd(T) ? e2 : e1);
            const int32_t i2 = ts_vertex_index<T>(a, v, sy, sz, ts_odd(T) ? e1 : e2);
            if (at < a.T) {
                a.triangles[(size_t)at * 3 + 0] = i0;
                a.triangles[(size_t)at * 3 + 1] = i1;
                a.triangles[(size_t)at * 3 + 2] = i2;
            }
            ++at;
        }
        ts_emit_tets<T + 1>(a, v, sy, sz, ins, at);
    }
}

__global__ void __launch_bounds__(TS_THREADS) tsdf_emit_triangles_kernel(const TsdfEmitArgs a) {
    int i0, j, k;
    if (!tsdf_brick(a.g, i0, j, k)) return;
    const int i = i0 + (int)(threadIdx.x & 63);
    if (i >= a.g.nx) return;
    const size_t sy = (size_t)a.g.nx, sz = (size_t)a.g.nx * a.g.ny, v = (size_t)k * sz + (size_t)j * sy + i;
    if (!a.tcnt[v] || i >= a.g.nx - 1 || j >= a.g.ny - 1 || k >= a.g.nz - 1) return;     // > 0 only for a valid cell inside the grid
    uint32_t obs, ins;
    ts_corners(a.cls, v, sy, sz, obs, ins);
    uint32_t at = a.tloc[v] + a.tblk[v >> TS_SCAN_SHIFT];
    ts_emit_tets<0>(a, v, sy, sz, ins, at);
}

}  // namespace mgs

using namespace mgs;

extern "C" {

static int tsdf_volume_error(const char* who, const mgs_tsdf_volume* vol) {
    if (!vol) { set_error("%s: volume must be non-NULL", who); return 1; }
    if (vol->nx <= 0 || vol->ny <= 0 || vol->nz <= 0) { set_error("%s: grid dimensions must be positive", who); return 1; }
    if ((uint64_t)vol->nx * (uint64_t)vol->ny * (uint64_t)vol->nz >= ((uint64_t)1 << 31)) {
        set_error("%s: nx x ny x nz must stay below 2^31", who);
        return 1;
    }
    if (!(vol->voxel > 0.f)) { set_error("%s: voxel edge must be positive", who); return 1; }
    if (!vol->tsdf || !vol->weight) { set_error("%s: tsdf and weight planes must be non-NULL", who); return 1; }
    const int nc = (vol->r ? 1 : 0) + (vol->g ? 1 : 0) + (vol->b ? 1 : 0);
    if (nc != 0 && nc != 3) { set_error("%s: colour planes r, g, b: all three or none", who); return 1; }
    return 0;
}
static TsdfGrid tsdf_grid(const mgs_tsdf_volume* vol) {
    TsdfGrid g;
    g.nx = vol->nx; g.ny = vol->ny; g.nz = vol->nz; g.xchunks = (vol->nx + WAVE - 1) / WAVE;
    g.ox = vol->origin[0]; g.oy = vol->origin[1]; g.oz = vol->origin[2]; g.s = vol->voxel;
    return g;
}

int mgs_tsdf_integrate(const mgs_tsdf_volume* vol, const mgs_tsdf_frame* fr, void* stream) {
    const char* who = "mgs_tsdf_integrate";
    if (tsdf_volume_error(who, vol)) return 1;
    if (!fr) { set_error("%s: frame must be non-NULL", who); return 1; }
    if (fr->width <= 0 || fr->height <= 0) { set_error("%s: image size must be positive", who); return 1; }
    if ((size_t)fr->width * fr->height >= ((size_t)1 << 31)) { set_error("%s: width x height must stay below 2^31", who); return 1; }
    if (!fr->depth || !fr->viewmatrix) { set_error("%s: depth and viewmatrix must be non-NULL", who); return 1; }
    if (!(fr->trunc > 0.f)) { set_error("%s: trunc must be positive", who); return 1; }
    if (!(fr->max_weight >= 1.f)) { set_error("%s: max_weight must be at least 1", who); return 1; }
    if (!(fr->fx > 0.f) || !(fr->fy > 0.f)) { set_error("%s: fx and fy must be positive", who); return 1; }
    TsdfIntegrateArgs a;
    a.g = tsdf_grid(vol);
    a.tsdf = vol->tsdf; a.weight = vol->weight; a.r = vol->r; a.gr = vol->g; a.b = vol->b;
    a.depth = fr->depth; a.opacity = fr->opacity; a.rgb = fr->rgb; a.view = fr->viewmatrix;
    a.W = fr->width; a.H = fr->height;
    a.fx = fr->fx; a.fy = fr->fy; a.cx = fr->cx; a.cy = fr->cy;
    a.trunc = fr->trunc; a.depth_min = fr->depth_min; a.depth_max = fr->depth_max; a.opacity_min = fr->opacity_min;
    a.max_weight = fr->max_weight;
    a.cull = (fr->flags & MGS_TSDF_NO_CULL) ? 0 : 1;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(tsdf_blocks(a.g)), dim3(TS_THREADS), 0, (hipStream_t)stream, a);
    MGS_HIP(hipGetLastError());
    return 0;
}

size_t mgs_tsdf_extract_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0 || (uint64_t)nx * (uint64_t)ny * (uint64_t)nz >= ((uint64_t)1 << 31)) return 256;
    return tsdf_carve(nullptr, (size_t)nx * ny * nz).bytes;
}

int mgs_tsdf_extract_count(const mgs_tsdf_volume* vol, float min_weight, void* scratch, uint32_t* counts, void* stream) {
    const char* who = "mgs_tsdf_extract_count";
    if (tsdf_volume_error(who, vol)) return 1;
    if (!scratch || !counts) { set_error("%s: scratch and counts must be non-NULL", who); return 1; }
    const TsdfGrid g = tsdf_grid(vol);
    const size_t N = (size_t)g.nx * g.ny * g.nz;
    const TsdfScratch sc = tsdf_carve(scratch, N);
    const unsigned nb = (unsigned)(align_up(N, TS_SCAN_ITEMS) / TS_SCAN_ITEMS);
    hipStream_t s = (hipStream_t)stream;
    size_t cb = (N + TS_THREADS - 1) / TS_THREADS;
    cb = cb > 8192 ? 8192 : cb;
    hipLaunchKernelGGL(tsdf_classify_kernel, dim3((unsigned)cb), dim3(TS_THREADS), 0, s, vol->tsdf, vol->weight, min_weight, N, sc.cls);
    hipLaunchKernelGGL(tsdf_cells_kernel, dim3(tsdf_blocks(g)), dim3(TS_THREADS), 0, s, g, sc.cls, sc.valid, sc.tcnt);
    hipLaunchKernelGGL(tsdf_edges_kernel, dim3(tsdf_blocks(g)), dim3(TS_THREADS), 0, s, g, sc.cls, sc.valid, sc.emask);
    hipLaunchKernelGGL(tsdf_scan_local_kernel, dim3(nb, 2), dim3(TS_THREADS), 0, s, sc.emask, sc.tcnt, sc.vloc, sc.tloc, sc.vblk,
                       sc.tblk, N);
    hipLaunchKernelGGL(tsdf_scan_blocks_kernel, dim3(2), dim3(TS_SCANB_THREADS), 0, s, sc.vblk, sc.tblk, nb, counts);
    MGS_HIP(hipGetLastError());
    return 0;
}

int mgs_tsdf_extract_emit(const mgs_tsdf_volume* vol, const void* scratch, float* vertices, float* colors, int32_t* triangles,
                          uint32_t V, uint32_t T, void* stream) {
    const char* who = "mgs_tsdf_extract_emit";
    if (tsdf_volume_error(who, vol)) return 1;
    if (!scratch) { set_error("%s: scratch must be non-NULL", who); return 1; }
    if (V >= (1u << 31) || T >= (1u << 31)) { set_error("%s: V and T must stay below 2^31", who); return 1; }
    if ((V && !vertices) || (T && !triangles)) { set_error("%s: vertices and triangles must be non-NULL", who); return 1; }
    if (colors && !vol->r) { set_error("%s: colors given for a volume without colour planes", who); return 1; }
    if (V == 0 && T == 0) return 0;
    TsdfEmitArgs a;
    a.g = tsdf_grid(vol);
    const TsdfScratch sc = tsdf_carve(const_cast<void*>(scratch), (size_t)a.g.nx * a.g.ny * a.g.nz);
    a.tsdf = vol->tsdf; a.r = vol->r; a.gr = vol->g; a.b = vol->b;
    a.cls = sc.cls; a.emask = sc.emask; a.tcnt = sc.tcnt;
    a.vloc = sc.vloc; a.tloc = sc.tloc; a.vblk = sc.vblk; a.tblk = sc.tblk;
    a.vertices = vertices; a.colors = colors; a.triangles = triangles; a.V = V; a.T = T;
    hipStream_t s = (hipStream_t)stream;
    if (V) hipLaunchKernelGGL(tsdf_emit_vertices_kernel, dim3(tsdf_blocks(a.g)), dim3(TS_THREADS), 0, s, a);
    if (T) hipLaunchKernelGGL(tsdf_emit_triangles_kernel, dim3(tsdf_blocks(a.g)), dim3(TS_THREADS), 0, s, a);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
