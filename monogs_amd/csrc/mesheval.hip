// Reconstruction evaluation against a ground-truth mesh: cross-set nearest neighbour, area-weighted stratified mesh sampling, the
// per-vertex visibility cull and the reduction to the figures.  The specification is DESIGN.md, "Reconstruction evaluation";
// tests/mesh_eval_mirror.py restates it in float64.  No counterpart in the reference (it has no mesh); nothing here is ported.
//
// Every entry point takes a stream, keeps no state between calls, uses no float atomics and no library kernels, and is bitwise
// reproducible from call to call: minima and integer sums do not depend on order, the double sums are taken in a fixed order.
//
// mgs_nn_dist2, two paths, bit-identical in d2 and index (a minimum of the same float32 numbers, ties to the smaller index):
//   * P < KNN_GRID_MIN targets: an LDS-tiled all-pairs sweep, one query per lane, tiles of 1024 targets read back as broadcasts
//     (knn_kernel's shape).  The threshold is the one knn.hip measured for its own two paths (6144): per query both pairs of
//     paths trade the same P pair tests against the same sort + index build.
//   * more targets: the Morton-box index of knn.hip over the JOINT bounding box of queries and targets, built once for the targets
//     (boxes of 64 with bounds) and once for the queries (so that a wave's 64 queries are neighbours; their box bounds are the
//     wave's own bounds).  One wave answers 64 queries: it seeds its bound from the target box where its first query's code falls
//     (binary search in the sorted target codes) and that box's two neighbours along the curve, prunes 64 candidate boxes at a time
//     wave-uniformly against its own bounds and the largest current best of its lanes, and stages the survivors through LDS.
//     A box is dropped only when its lower bound EXCEEDS the best (<= keeps it): a box that could tie may hold the smaller index.
#include "common.h"

namespace mgs {

constexpr int NN_THREADS = 256;
constexpr int NN_TILE = 1024;

// one candidate against the running (best, index): smaller distance, or the same distance at a smaller index
__device__ __forceinline__ void nn_take(float d, int ti, float& best, int& bi) {
    const bool better = d < best || (d == best && ti < bi);
    best = better ? d : best;
    bi = better ? ti : bi;
}

__global__ void __launch_bounds__(NN_THREADS) nn_all_pairs_kernel(int Q, int P, const float* __restrict__ qs, const float* __restrict__ ts,
                                                                  float* __restrict__ d2, int32_t* __restrict__ index) {
    __shared__ float4 tile[NN_TILE];
    const int idx = blockIdx.x * NN_THREADS + threadIdx.x;
    const bool live = idx < Q;
    const float qx = live ? qs[3 * (size_t)idx] : 0.f, qy = live ? qs[3 * (size_t)idx + 1] : 0.f, qz = live ? qs[3 * (size_t)idx + 2] : 0.f;
    float best = __int_as_float(0x7f800000);
    int bi = -1;
    for (int start = 0; start < P; start += NN_TILE) {
        const int n = min(NN_TILE, P - start);
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += NN_THREADS) {
            const size_t s = (size_t)(start + i);
            tile[i] = make_float4(ts[3 * s], ts[3 * s + 1], ts[3 * s + 2], 0.f);
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            const float4 c = tile[i];
            nn_take(pair_d2(c.x, c.y, c.z, qx, qy, qz), start + i, best, bi);
        }
    }
    if (live) {
        d2[idx] = best;
        if (index) index[idx] = bi;
    }
}

struct NnQueryArgs {
    int Q, P, nbq, nbt;
    const float4 *qsorted, *qlo, *qhi;         // the queries' index: sorted points, bounds of each run of 64
    const uint32_t* qcode;                     // their sorted codes
    const float4 *tsorted, *tlo, *thi;         // the targets' index
    const uint32_t* tcode;
    float* d2;
    int32_t* index;
};

// the cross-set policy of the walk (morton_box_walk, common.h): one best with the smaller index; a box is dropped only when its
// lower bound EXCEEDS the best (<= keeps it), since a box that could tie may hold the smaller index
struct NnBest1 {
    const NnQueryArgs& a;
    int qb;
    float best;
    int bi;
    __device__ __forceinline__ void take(const float4& c, const float4& q, int, int) {
        nn_take(pair_d2(c.x, c.y, c.z, q.x, q.y, q.z), (int)__float_as_uint(c.w), best, bi);
    }
    __device__ __forceinline__ float bound() const { return best; }
    __device__ __forceinline__ void store(const float4& q) const {
        const uint32_t o = __float_as_uint(q.w);                     // back in the caller's order
        a.d2[o] = best;
        if (a.index) a.index[o] = bi;
    }
    static __device__ __forceinline__ bool keep(float lower, float bound) { return lower <= bound; }
    // the target box where the wave's first query falls along the curve (first sorted target code >= its code), and its neighbours
    template <typename Sweep>
    __device__ __forceinline__ int seed(Sweep&& sweep) {
        const uint32_t code0 = a.qcode[qb * KNN_BOX];
        int hi = a.P, lo = 0;                    // (hi first: the other order exchanges the operands of the midpoint's add)
        while (lo < hi) {
            const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
            if (a.tcode[mid] < code0) lo = mid + 1;
            else hi = mid;
        }
        const int sb = __builtin_amdgcn_readfirstlane(min(lo, a.P - 1) / KNN_BOX);
        sweep(sb);
        if (sb + 1 < a.nbt) sweep(sb + 1);
        if (sb > 0) sweep(sb - 1);
        return sb;
    }
};

__global__ void __launch_bounds__(NN_THREADS) nn_query_kernel(const NnQueryArgs a) {
    __shared__ float4 cand[NN_THREADS / 64][KNN_BOX];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qb = blockIdx.x * (NN_THREADS / 64) + wv;             // this wave's run of 64 queries
    if (qb >= a.nbq) return;                                        // whole wave; no block-level barrier below
    const int qi = qb * KNN_BOX + lane;
    const bool live = qi < a.Q;
    const float4 q = a.qsorted[live ? qi : a.Q - 1];
    const float4 qlo = a.qlo[qb], qhi = a.qhi[qb];
    NnBest1 r{a, qb, __int_as_float(0x7f800000), -1};
    morton_box_walk(r, a.P, a.nbt, a.tsorted, a.tlo, a.thi, q, qlo, qhi, live, lane, cand, wv);
}

__global__ void __launch_bounds__(NN_THREADS) nn_empty_kernel(int Q, float* __restrict__ d2, int32_t* __restrict__ index) {
    const int i = blockIdx.x * NN_THREADS + threadIdx.x;
    if (i >= Q) return;
    d2[i] = __int_as_float(0x7f800000);
    if (index) index[i] = -1;
}

struct NnScratch { MortonIndex t, q; size_t bytes; };
static NnScratch nn_carve(void* base, int Q, int P) {
    NnScratch s;
    ScratchCursor c(base);
    s.t = morton_carve(c.p0, P);
    s.q = morton_carve(c.p0 + s.t.bytes, Q);
    s.bytes = s.t.bytes + s.q.bytes + 256;
    return s;
}

// ---- mesh sampling ------------------------------------------------------------------------------------------------------------
constexpr int MS_THREADS = 256;
constexpr int MS_SCAN_ITEMS = 2048;             // per scan block: 256 threads x 8 consecutive triangles (tsdf.hip's scan shape)
constexpr int MS_SCAN_SHIFT = 11;
constexpr int MS_SCANB_THREADS = 1024;

struct MeshSampleScratch {
    int32_t* bbox;            // [8] the vertices' bounding box (ordered ints, as the Morton index keeps it)
    uint64_t* incl;           // [Tp] quantised areas, then their inclusive sums inside each scan block
    uint64_t* blk;            // [nb] exclusive scan of the block sums
    uint64_t* total;          // [1]
    size_t bytes;
};
static MeshSampleScratch ms_carve(void* base, size_t T) {
    const size_t Tp = align_up(T ? T : 1, MS_SCAN_ITEMS), nb = Tp / MS_SCAN_ITEMS;
    ScratchCursor c(base);
    MeshSampleScratch s;
    s.bbox = c.take<int32_t>(8 * sizeof(int32_t));
    s.incl = c.take<uint64_t>(Tp * 8);
    s.blk = c.take<uint64_t>(nb * 8);
    s.total = c.take<uint64_t>(8);
    s.bytes = c.used() + ScratchCursor::ALIGN;
    return s;
}

// The fixed-point scale of the areas, a power of two: with D2 the squared diagonal of the vertices' bounding box no triangle is
// larger than D2 / 2 < 2^(eD - 1) and T <= 2^eT, so every sum of areas stays below 2^(eT + eD - 1); the scale 2^(61 - eT - eD)
// keeps the quantised total below 2^60 (the spare bits: float32 rounding of the areas).  Every thread forms it from the same six
// numbers: the same value everywhere.
__device__ __forceinline__ double ms_scale(const int32_t* __restrict__ bbox, int T) {
    double d2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double e = (double)ord2f(bbox[4 + a]) - (double)ord2f(bbox[a]);
        d2 += e * e;
    }
    int eD = 0, eT = 0;
    if (d2 > 0.0 && d2 < 1e300) frexp(d2, &eD);          // d2 < 2^eD
    while ((1u << eT) < (uint32_t)T && eT < 31) ++eT;      // T <= 2^eT
    int e = 61 - eT - eD;
    e = e > 1000 ? 1000 : (e < -1000 ? -1000 : e);
    return ldexp(1.0, e);
}

__global__ void __launch_bounds__(MS_THREADS) mesh_area_kernel(int V, int T, const float* __restrict__ vert, const int32_t* __restrict__ tri,
                                                               const uint8_t* __restrict__ keep, const int32_t* __restrict__ bbox,
                                                               uint64_t* __restrict__ area_q, uint32_t* __restrict__ status) {
    const int t = blockIdx.x * MS_THREADS + threadIdx.x;
    if (t >= T) return;
    const int ia = tri[3 * (size_t)t], ib = tri[3 * (size_t)t + 1], ic = tri[3 * (size_t)t + 2];
    uint64_t q = 0ull;
    if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) {
        atomicOr(status, 1u);                                       // an argument error: nothing is read through the index
    } else if (!keep || keep[t]) {
        const float ax = vert[3 * (size_t)ia], ay = vert[3 * (size_t)ia + 1], az = vert[3 * (size_t)ia + 2];
        const float ux = vert[3 * (size_t)ib] - ax, uy = vert[3 * (size_t)ib + 1] - ay, uz = vert[3 * (size_t)ib + 2] - az;
        const float vx = vert[3 * (size_t)ic] - ax, vy = vert[3 * (size_t)ic + 1] - ay, vz = vert[3 * (size_t)ic + 2] - az;
        const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const float area = 0.5f * sqrtf(nx * nx + ny * ny + nz * nz);
        if (area > 0.f && area < __int_as_float(0x7f800000)) {
            const double x = (double)area * ms_scale(bbox, T);
            q = x < 1152921504606846976.0 ? (uint64_t)x : 0ull;     // (2^60: beyond it the vertices were not inside the box)
        }
    }
    area_q[t] = q;
}

// block-local inclusive scan in place; a thread owns 8 consecutive items, items at index >= T count as 0
__global__ void __launch_bounds__(MS_THREADS) mesh_scan_local_kernel(uint64_t* __restrict__ incl, uint64_t* __restrict__ blk, int T) {
    __shared__ uint64_t s_w[MS_THREADS / WAVE];
    const size_t base = (size_t)blockIdx.x * MS_SCAN_ITEMS + (size_t)threadIdx.x * 8;
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
    for (int w = 0; w < MS_THREADS / WAVE; ++w) {
        before += w < wv ? s_w[w] : 0ull;
        total += s_w[w];
    }
#pragma unroll
    for (int n = 0; n < 8; ++n) incl[base + n] = x[n] + before;      // (the scratch holds whole scan blocks)
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the block sums in place, the grand total, and the kept area in square metres
__global__ void __launch_bounds__(MS_SCANB_THREADS) mesh_scan_blocks_kernel(uint64_t* __restrict__ blk, uint32_t nb, uint64_t* __restrict__ total_out,
                                                                            const int32_t* __restrict__ bbox, int T, double* __restrict__ area_out) {
    __shared__ uint64_t s_w[MS_SCANB_THREADS / WAVE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t carry = 0ull;
    for (uint32_t b0 = 0; b0 < nb; b0 += MS_SCANB_THREADS) {
        const uint32_t b = b0 + threadIdx.x;
        const uint64_t x = b < nb ? blk[b] : 0ull;
        const uint64_t in = wave_incl_scan_u64(x, lane);
        if (lane == 63) s_w[wv] = in;
        __syncthreads();
        uint64_t before = carry, total = 0ull;
        for (int w = 0; w < MS_SCANB_THREADS / WAVE; ++w) {
            before += w < wv ? s_w[w] : 0ull;
            total += s_w[w];
        }
        before += in - x;
        if (b < nb) blk[b] = before;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        total_out[0] = carry;
        if (area_out) area_out[0] = (double)carry / ms_scale(bbox, T);
    }
}

// the counter-based hash: uniform k = 0, 1, 2 of sample s is the top 24 bits of mix(mix(seed ^ 0x9E3779B9) + 3 s + k)
__device__ __forceinline__ uint32_t ms_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__global__ void __launch_bounds__(MS_THREADS) mesh_sample_kernel(int T, int N, uint32_t seed, const float* __restrict__ vert,
                                                                 const int32_t* __restrict__ tri, const uint64_t* __restrict__ incl,
                                                                 const uint64_t* __restrict__ blk, const uint64_t* __restrict__ total_p,
                                                                 float* __restrict__ points, int32_t* __restrict__ tri_index) {
    const int s = blockIdx.x * MS_THREADS + threadIdx.x;
    if (s >= N) return;
    const uint64_t total = total_p[0];
    if (total == 0ull) {                                              // no kept area: the wrapper reports it; nothing to place
        points[3 * (size_t)s] = points[3 * (size_t)s + 1] = points[3 * (size_t)s + 2] = 0.f;
        if (tri_index) tri_index[s] = -1;
        return;
    }
    const uint32_t h0 = ms_mix(seed ^ 0x9E3779B9u) + 3u * (uint32_t)s;
    const float r0 = (float)(ms_mix(h0) >> 8) * 5.9604644775390625e-8f;
    const float r1 = (float)(ms_mix(h0 + 1u) >> 8) * 5.9604644775390625e-8f;
    const float r2 = (float)(ms_mix(h0 + 2u) >> 8) * 5.9604644775390625e-8f;
    const double x = ((double)s + (double)r0) / (double)N * (double)total;    // the stratum coordinate
    uint64_t u = (uint64_t)x;
    u = u < total ? u : total - 1ull;
    int lo = 0, hi = T - 1;                                           // the first triangle whose inclusive sum exceeds u (the last one's is total > u)
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (incl[mid] + blk[mid >> MS_SCAN_SHIFT] > u) hi = mid;
        else lo = mid + 1;
    }
    const int ia = tri[3 * (size_t)lo], ib = tri[3 * (size_t)lo + 1], ic = tri[3 * (size_t)lo + 2];   // (in range: its area is positive)
    const float ax = vert[3 * (size_t)ia], ay = vert[3 * (size_t)ia + 1], az = vert[3 * (size_t)ia + 2];
    const float su = sqrtf(r1), wb = su * (1.f - r2), wc = su * r2;
    points[3 * (size_t)s] = ax + wb * (vert[3 * (size_t)ib] - ax) + wc * (vert[3 * (size_t)ic] - ax);
    points[3 * (size_t)s + 1] = ay + wb * (vert[3 * (size_t)ib + 1] - ay) + wc * (vert[3 * (size_t)ic + 1] - ay);
    points[3 * (size_t)s + 2] = az + wb * (vert[3 * (size_t)ib + 2] - az) + wc * (vert[3 * (size_t)ic + 2] - az);
    if (tri_index) tri_index[s] = lo;
}

// ---- the visibility cull ------------------------------------------------------------------------------------------------------
struct MarkSeenArgs {
    int V, W, H;
    const float *vert, *view, *depth;         // depth may be NULL
    float fx, fy, cx, cy, depth_min, depth_max, eps;
    uint8_t* seen;
};

__global__ void __launch_bounds__(256) mesh_mark_seen_kernel(const MarkSeenArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.V) return;
    const ViewRows cam(MGS_CONST(a.view));
    const float px = a.vert[3 * (size_t)i], py = a.vert[3 * (size_t)i + 1], pz = a.vert[3 * (size_t)i + 2];
    // the transform, projection and pixel rule of tsdf_integrate_kernel (tsdf.hip): the same two statements
    MGS_TO_CAMERA(cam, px, py, pz, x, y, z);
    if (!(z > 0.f && z >= a.depth_min) || (a.depth_max > 0.f && z > a.depth_max)) return;
    size_t pix;
    if (!camera_pixel(a.fx, a.fy, a.cx, a.cy, a.W, a.H, x, y, z, pix)) return;
    if (a.depth) {
        const float d = a.depth[pix];
        if (!(d > 0.f) || !(z <= d + a.eps)) return;
    }
    a.seen[i] = 1;                                                    // the lane owns its byte: a plain store, earlier views stay
}

// ---- the figures ----------------------------------------------------------------------------------------------------------------
constexpr int RM_THREADS = 256;
constexpr int RM_MAX_BLOCKS = 256;
constexpr int RM_SLOTS = 2 + MGS_RECON_MAX_THRESHOLDS;     // sum, finite count, counts below each threshold
struct ReconArgs {
    int Q, K;
    const float* d2;
    float thr[MGS_RECON_MAX_THRESHOLDS];
    double* partial;          // [RM_MAX_BLOCKS][RM_SLOTS]
    double* out;              // [2 + K]
};

// sums of the block's RM_SLOTS values in a fixed order (wave butterfly, then waves 0..3): thread 0 holds them
__device__ __forceinline__ void rm_block_sum(double (&v)[RM_SLOTS], double (*s_w)[RM_SLOTS]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < RM_SLOTS; ++k) {
        v[k] = wave_sum(v[k]);
        if (lane == 0) s_w[wv][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < RM_SLOTS; ++k) {
            double t = 0.0;
            for (int w = 0; w < RM_THREADS / 64; ++w) t += s_w[w][k];
            v[k] = t;
        }
    }
}

__global__ void __launch_bounds__(RM_THREADS) recon_partial_kernel(const ReconArgs a) {
    __shared__ double s_w[RM_THREADS / 64][RM_SLOTS];
    double v[RM_SLOTS];
    unsigned cnt[RM_SLOTS];
#pragma unroll
    for (int k = 0; k < RM_SLOTS; ++k) { v[k] = 0.0; cnt[k] = 0u; }
    for (int i = blockIdx.x * RM_THREADS + threadIdx.x; i < a.Q; i += gridDim.x * RM_THREADS) {
        const float f = a.d2[i];
        if (!(fabsf(f) < __int_as_float(0x7f800000))) continue;      // +inf (no target) and NaN do not count
        const double d = sqrt((double)f);
        v[0] += d;
        cnt[1] += 1u;
#pragma unroll
        for (int k = 0; k < MGS_RECON_MAX_THRESHOLDS; ++k) cnt[2 + k] += (k < a.K && d < (double)a.thr[k]) ? 1u : 0u;
    }
#pragma unroll
    for (int k = 1; k < RM_SLOTS; ++k) v[k] = (double)cnt[k];        // integers below 2^53: their double sums are exact
    rm_block_sum(v, s_w);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < RM_SLOTS; ++k) a.partial[(size_t)blockIdx.x * RM_SLOTS + k] = v[k];
    }
}

__global__ void __launch_bounds__(RM_THREADS) recon_finish_kernel(const ReconArgs a, int nblocks) {
    __shared__ double s_w[RM_THREADS / 64][RM_SLOTS];
    double v[RM_SLOTS];
#pragma unroll
    for (int k = 0; k < RM_SLOTS; ++k) v[k] = (int)threadIdx.x < nblocks ? a.partial[(size_t)threadIdx.x * RM_SLOTS + k] : 0.0;
    rm_block_sum(v, s_w);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < RM_SLOTS; ++k)
            if (k < 2 + a.K) a.out[k] = v[k];
    }
}
static_assert(RM_MAX_BLOCKS <= RM_THREADS, "the finishing block reads one partial row per thread");

}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_nn_grid_min(void) { return KNN_GRID_MIN; }

size_t mgs_nn_scratch_bytes(int32_t Q, int32_t P) {
    if (Q <= 0 || P <= 0) return 256;
    return nn_carve(nullptr, Q, P).bytes;                  // sized for either path, whatever the flags say later
}

int mgs_nn_dist2(int32_t Q, int32_t P, const float* queries, const float* targets, int32_t flags, float* d2, int32_t* index,
                 void* scratch, void* stream) {
    const char* who = "mgs_nn_dist2";
    if (Q < 0 || P < 0) { set_error("%s: Q and P must not be negative", who); return 1; }
    if (Q > (1 << 30) || P > (1 << 30)) { set_error("%s: Q and P must stay within 2^30", who); return 1; }
    if (flags & ~(MGS_NN_FORCE_ALL_PAIRS | MGS_NN_FORCE_MORTON)) { set_error("%s: unknown flags", who); return 1; }
    if ((flags & MGS_NN_FORCE_ALL_PAIRS) && (flags & MGS_NN_FORCE_MORTON)) { set_error("%s: both paths forced", who); return 1; }
    if (Q == 0) return 0;
    if (!queries || !d2 || (P > 0 && !targets)) { set_error("%s: queries, targets and d2 must be non-NULL", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    const unsigned qblocks = (unsigned)((Q + NN_THREADS - 1) / NN_THREADS);
    if (P == 0) {
        hipLaunchKernelGGL(nn_empty_kernel, dim3(qblocks), dim3(NN_THREADS), 0, s, Q, d2, index);
        MGS_HIP(hipGetLastError());
        return 0;
    }
    const bool morton = (flags & MGS_NN_FORCE_MORTON) || (!(flags & MGS_NN_FORCE_ALL_PAIRS) && P >= KNN_GRID_MIN);
    if (!morton) {
        hipLaunchKernelGGL(nn_all_pairs_kernel, dim3(qblocks), dim3(NN_THREADS), 0, s, Q, P, queries, targets, d2, index);
        MGS_HIP(hipGetLastError());
        return 0;
    }
    if (!scratch) { set_error("%s: scratch is NULL", who); return 1; }
    const NnScratch k = nn_carve(scratch, Q, P);
    int32_t* bbox = k.t.bbox;                              // the joint box of both sets
    morton_bbox_reset(bbox, s);
    morton_bbox_extend(P, targets, bbox, s);
    morton_bbox_extend(Q, queries, bbox, s);
    NnQueryArgs a;
    if (int rc = morton_build(P, targets, bbox, k.t, s, &a.tcode)) return rc;
    if (int rc = morton_build(Q, queries, bbox, k.q, s, &a.qcode)) return rc;
    a.Q = Q; a.P = P; a.nbq = (Q + KNN_BOX - 1) / KNN_BOX; a.nbt = (P + KNN_BOX - 1) / KNN_BOX;
    a.qsorted = k.q.sorted; a.qlo = k.q.box_lo; a.qhi = k.q.box_hi;
    a.tsorted = k.t.sorted; a.tlo = k.t.box_lo; a.thi = k.t.box_hi;
    a.d2 = d2; a.index = index;
    hipLaunchKernelGGL(nn_query_kernel, dim3((unsigned)((a.nbq + 3) / 4)), dim3(NN_THREADS), 0, s, a);
    MGS_HIP(hipGetLastError());
    return 0;
}

size_t mgs_mesh_sample_scratch_bytes(int32_t T) { return ms_carve(nullptr, T > 0 ? (size_t)T : 0).bytes; }

int mgs_mesh_sample(int32_t V, int32_t T, const float* vertices, const int32_t* triangles, const uint8_t* keep, int32_t N,
                    uint32_t seed, float* points, int32_t* tri_index, double* area, uint32_t* status, void* scratch, void* stream) {
    const char* who = "mgs_mesh_sample";
    if (V <= 0 || T <= 0) { set_error("%s: the mesh needs vertices and triangles", who); return 1; }
    if (N < 0) { set_error("%s: N must not be negative", who); return 1; }
    if (V > (1 << 30) || T > (1 << 30) || N > (1 << 30)) { set_error("%s: V, T and N must stay within 2^30", who); return 1; }
    if (!vertices || !triangles || !status || !scratch || (N > 0 && !points)) {
        set_error("%s: vertices, triangles, points, status and scratch must be non-NULL", who);
        return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    const MeshSampleScratch k = ms_carve(scratch, (size_t)T);
    const unsigned nb = (unsigned)(align_up((size_t)T, MS_SCAN_ITEMS) / MS_SCAN_ITEMS);
    morton_bbox_reset(k.bbox, s);
    morton_bbox_extend(V, vertices, k.bbox, s);
    hipLaunchKernelGGL(mesh_area_kernel, dim3((unsigned)((T + MS_THREADS - 1) / MS_THREADS)), dim3(MS_THREADS), 0, s, V, T, vertices, triangles,
                       keep, k.bbox, k.incl, status);
    hipLaunchKernelGGL(mesh_scan_local_kernel, dim3(nb), dim3(MS_THREADS), 0, s, k.incl, k.blk, T);
    hipLaunchKernelGGL(mesh_scan_blocks_kernel, dim3(1), dim3(MS_SCANB_THREADS), 0, s, k.blk, nb, k.total, k.bbox, T, area);
    if (N > 0)
        hipLaunchKernelGGL(mesh_sample_kernel, dim3((unsigned)((N + MS_THREADS - 1) / MS_THREADS)), dim3(MS_THREADS), 0, s, T, N, seed, vertices,
                           triangles, k.incl, k.blk, k.total, points, tri_index);
    MGS_HIP(hipGetLastError());
    return 0;
}

int mgs_mesh_mark_seen(int32_t V, const float* vertices, const float* viewmatrix, int32_t W, int32_t H, float fx, float fy, float cx,
                       float cy, const float* depth, float depth_min, float depth_max, float occlusion_eps, uint8_t* seen, void* stream) {
    const char* who = "mgs_mesh_mark_seen";
    if (V < 0) { set_error("%s: V must not be negative", who); return 1; }
    if (W <= 0 || H <= 0 || (size_t)W * H >= ((size_t)1 << 31)) { set_error("%s: image size must be positive and below 2^31 pixels", who); return 1; }
    if (!(fx > 0.f) || !(fy > 0.f)) { set_error("%s: fx and fy must be positive", who); return 1; }
    if (V == 0) return 0;
    if (!vertices || !viewmatrix || !seen) { set_error("%s: vertices, viewmatrix and seen must be non-NULL", who); return 1; }
    MarkSeenArgs a;
    a.V = V; a.W = W; a.H = H; a.vert = vertices; a.view = viewmatrix; a.depth = depth;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.depth_min = depth_min; a.depth_max = depth_max; a.eps = occlusion_eps; a.seen = seen;
    hipLaunchKernelGGL(mesh_mark_seen_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    MGS_HIP(hipGetLastError());
    return 0;
}

size_t mgs_recon_metrics_scratch_bytes(void) { return (size_t)RM_MAX_BLOCKS * RM_SLOTS * sizeof(double) + 256; }

int mgs_recon_metrics(int32_t Q, const float* d2, int32_t K, const float* thresholds, double* out, void* scratch, void* stream) {
    const char* who = "mgs_recon_metrics";
    if (Q < 0 || K < 0 || K > MGS_RECON_MAX_THRESHOLDS) { set_error("%s: Q >= 0 and 0 <= K <= %d", who, MGS_RECON_MAX_THRESHOLDS); return 1; }
    if (!out || !scratch || (Q > 0 && !d2) || (K > 0 && !thresholds)) { set_error("%s: d2, thresholds, out and scratch must be non-NULL", who); return 1; }
    ReconArgs a;
    a.Q = Q; a.K = K; a.d2 = d2; a.out = out;
    a.partial = (double*)align_up((size_t)scratch, 256);
    for (int k = 0; k < MGS_RECON_MAX_THRESHOLDS; ++k) a.thr[k] = k < K ? thresholds[k] : 0.f;
    hipStream_t s = (hipStream_t)stream;
    int blocks = (Q + RM_THREADS * 4 - 1) / (RM_THREADS * 4);        // about four entries per thread
    blocks = blocks > RM_MAX_BLOCKS ? RM_MAX_BLOCKS : blocks;
    if (blocks) hipLaunchKernelGGL(recon_partial_kernel, dim3((unsigned)blocks), dim3(RM_THREADS), 0, s, a);
    hipLaunchKernelGGL(recon_finish_kernel, dim3(1), dim3(RM_THREADS), 0, s, a, blocks);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
