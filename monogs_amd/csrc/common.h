// Internal definitions shared by the HIP translation units of libmonogs_raster.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/monogs_raster.h"
#include "wave_ops.h"          // wave reductions and scans, the reproducible workgroup sums
#include "forward_plan.h"      // ForwardPlan: the forward's route decisions, read by every stage launcher

namespace mgs {

constexpr int TILE = MGS_TILE;          // 16x16 pixel tiles define the binning tables
constexpr int WAVE = 64;                // gfx950 wavefront
constexpr int SUB = 8;                  // one wave blends an 8x8 quadrant of a tile
constexpr int REC_FLOATS = 16;          // per-Gaussian blend record: one 64-byte line
constexpr int GRAD_FLOATS = 16;         // per-Gaussian gradient accumulator: one 64-byte line

// blend record slots (float index inside the 64-byte record written by preprocess):
//   float4 #0 {px, py, ex, ey}   what a lane needs for the quadrant cull test
//   float4 #1 {ka, kb, kc, opacity}      } fetched with scalar loads for a surviving instance;
//                                          (ka, kb, kc) = (-log2e/2 a, -log2e b, -log2e/2 c) of the conic, so that
//                                          alpha = opacity * exp2(ka dx^2 + kb dx dy + kc dy^2): 5 VALU ops + v_exp_f32
//   float4 #2 {r, g, b, depth}           }
//   float4 #3 {na, nb, nc, radius}   conic / (2 ln(255 o)) for the exact ellipse-vs-quadrant cull test; radius for duplicate
enum : int {
    R_X = 0, R_Y = 1, R_EX = 2, R_EY = 3,
    R_CA = 4, R_CB = 5, R_CC = 6, R_OPAC = 7,
    R_R = 8, R_G = 9, R_B = 10, R_DEPTH = 11,
    R_NA = 12, R_NB = 13, R_NC = 14, R_RADIUS = 15
};
// gradient accumulator slots (float atomics by the blend backward).  With h = G * dL/dalpha summed
// over the pixels of every tile the Gaussian touches, the blend backward stores the RAW moments
//   S_X = sum h dx, S_Y = sum h dy, S_XX = sum h dx^2, S_XY = sum h dx dy, S_YY = sum h dy^2, S_H = sum h
// (d = mean2D - pixel); the per-Gaussian constants (conic, opacity, -1/2) are applied once per
// Gaussian in geom_backward instead of once per (pixel, instance) pair -- the map is linear.
enum : int {
    G_SX = 0, G_SY = 1, G_SXX = 2, G_SXY = 3, G_SYY = 4, G_SH = 5,
    G_DR = 6, G_DG = 7, G_DB = 8, G_DDEPTH = 9
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Host: a bump allocator over one scratch buffer, every sub-buffer 256-byte aligned (the feature units' scratch; the forward's
// named layout is api.hip's Carver).  The base is rounded up first; used() counts from the rounded base.
struct ScratchCursor {
    static constexpr size_t ALIGN = 256;
    char *p0, *p;
    explicit ScratchCursor(void* base) : p0((char*)align_up((size_t)base, ALIGN)), p(p0) {}
    template <typename T>
    T* take(size_t bytes) { char* r = p; p += align_up(bytes, ALIGN); return (T*)r; }
    size_t used() const { return (size_t)(p - p0); }
};

// Wave-uniform read-only inputs (camera matrices, background colour): read through the CONSTANT address space, so the
// backend always selects scalar loads (s_load_dwordx8/x16, all issued at once) for them.  Through a generic pointer
// it falls back to per-lane vector loads with a vmcnt(0) wait after each group as soon as the kernel also stores to
// global memory (its no-clobber analysis gives up): the per-Gaussian kernels spent seven dependent memory round trips
// on their 51 camera floats that way.  Valid because these buffers are written by an EARLIER kernel, never by the one
// reading them (kernel boundaries invalidate the scalar cache).
#if defined(__HIP_DEVICE_COMPILE__)
typedef const float __attribute__((address_space(4))) * const_float_p;
typedef const unsigned long long __attribute__((address_space(4))) * const_u64_p;
#define MGS_CONST(p) ((mgs::const_float_p)(p))
#define MGS_CONST_U64(p) ((mgs::const_u64_p)(p))
#else
typedef const float* const_float_p;
typedef const unsigned long long* const_u64_p;
#define MGS_CONST(p) (p)
#define MGS_CONST_U64(p) (p)
#endif

// ---- a world point to its pixel: the ONE rule of TSDF integration (tsdf.hip) and the mesh visibility cull (mesheval.hip) ----
// the rows of the world->camera transform, loaded from the transposed matrix of mgs_camera.viewmatrix
struct ViewRows {
    const float r00, r01, r02, tx, r10, r11, r12, ty, r20, r21, r22, tz;
    __device__ __forceinline__ explicit ViewRows(const_float_p vm)
        : r00(vm[0]), r01(vm[4]), r02(vm[8]), tx(vm[12]), r10(vm[1]), r11(vm[5]), r12(vm[9]), ty(vm[13]),
          r20(vm[2]), r21(vm[6]), r22(vm[10]), tz(vm[14]) {}
};
// declares x, y, z: the camera-space point of the world point (px, py, pz).  (A statement: as an inlined function it came out with
// the operands of two packed multiplies of tsdf_integrate_kernel exchanged.)
#define MGS_TO_CAMERA(cam, px, py, pz, x, y, z)                              \
    const float x = cam.r00 * px + cam.r01 * py + cam.r02 * pz + cam.tx,     \
                y = cam.r10 * px + cam.r11 * py + cam.r12 * pz + cam.ty,     \
                z = cam.r20 * px + cam.r21 * py + cam.r22 * pz + cam.tz
// the pixel whose centre is nearest to the projection of the camera-space point (x, y, z), z > 0; false: outside the image
__device__ __forceinline__ bool camera_pixel(float fx, float fy, float cx, float cy, int W, int H, float x, float y, float z,
                                             size_t& pix) {
    const float u = fx * x / z + cx - 0.5f, v = fy * y / z + cy - 0.5f;
    const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
    if (!(fu >= 0.f && fu < (float)W && fv >= 0.f && fv < (float)H)) return false;
    pix = (size_t)(int)fv * W + (int)fu;
    return true;
}

// ---- zero fill as a plain kernel ------------------------------------------------------------
// Every clear on the hot path is a kernel, never hipMemsetAsync / hipMemcpyAsync: inside a captured hipGraph
// those become memset / memcpy NODES, and on this ROCm a graph holding them faulted ("write access to a
// read-only page") once unrelated eager copies ran between two replays (tools/graph_probe.py).  Kernel nodes
// replay exactly as launched.  `ptr` must be 4-byte aligned and `bytes` a multiple of 4.
__global__ static void zero_fill_kernel(uint32_t* __restrict__ p, size_t n_words, int vec) {
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (vec) {
        uint4* q = reinterpret_cast<uint4*>(p);
        const size_t nv = n_words / 4;
        for (size_t i = i0; i < nv; i += stride) q[i] = make_uint4(0u, 0u, 0u, 0u);
        for (size_t i = nv * 4 + i0; i < n_words; i += stride) p[i] = 0u;
    } else {
        for (size_t i = i0; i < n_words; i += stride) p[i] = 0u;
    }
}
// the same clear, done by the threads of a kernel that runs anyway (p 16-byte aligned): saves a launch
// (`threads` = total threads of the launch, passed by the host: blockDim / gridDim would be fetched from the dispatch
//  packet with a vector load + wait, a memory round trip at the very start of the kernel)
__device__ __forceinline__ void grid_zero(uint32_t* __restrict__ p, size_t n_words, size_t threads, int block) {
    const size_t i0 = (size_t)blockIdx.x * block + threadIdx.x, stride = threads;
    uint4* q = reinterpret_cast<uint4*>(p);
    const size_t nv = n_words / 4;
    for (size_t i = i0; i < nv; i += stride) q[i] = make_uint4(0u, 0u, 0u, 0u);
    for (size_t i = nv * 4 + i0; i < n_words; i += stride) p[i] = 0u;
}
// two regions in one launch (the second one small): gradient accumulator + the 6 pose-gradient floats
__global__ static void zero_fill2_kernel(uint32_t* __restrict__ p, size_t n_words, uint32_t* __restrict__ p2, int n2) {
    grid_zero(p, n_words, (size_t)gridDim.x * 256, 256);
    if (blockIdx.x == 0 && (int)threadIdx.x < n2) p2[threadIdx.x] = 0u;
}
static inline hipError_t zero_fill2(void* ptr, size_t bytes, void* ptr2, size_t bytes2, hipStream_t s) {
    const size_t n_words = bytes / 4;                       // ptr 16-byte aligned; bytes2 <= 1 KiB
    size_t blocks = (n_words / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    hipLaunchKernelGGL(zero_fill2_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (uint32_t*)ptr, n_words,
                       (uint32_t*)ptr2, ptr2 ? (int)(bytes2 / 4) : 0);
    return hipGetLastError();
}
static inline hipError_t zero_fill(void* ptr, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    const size_t n_words = bytes / 4;
    const int vec = ((size_t)ptr % 16 == 0) ? 1 : 0;
    const size_t items = vec ? (n_words + 3) / 4 : n_words;
    size_t blocks = (items + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (uint32_t*)ptr, n_words, vec);
    return hipGetLastError();
}

// ---- scratch carving (the layouts themselves: api.hip; every sub-buffer of the forward 256-byte aligned) ----
struct GeometryState {
    float* rec;               // [P][16]
    uint32_t* depth_key;      // [P] float32 bits of the view-space depth (0xFFFFFFFF when culled); sort input
    uint32_t* depth_alt;      // [P] ping-pong partner of depth_key.  NOTE: depth_alt .. perm (contiguous) are ALSO the band tables of
                              //     the banded tile sort on the per-tile path, which runs no global depth sort (band_totals
                              //     below): whoever uses one of the four there must move those tables first
    uint32_t* iota;           // [P] ping-pong buffers of the depth sort's values (the first pass takes value = index and
    uint32_t* iota_alt;       // [P] reads neither)
    uint32_t* perm;           // [P] Gaussian index in (depth, index) order -- culled ones last: written by the sort's final pass
    uint32_t* point_offsets;  // [P] inclusive scan, in depth order, of the tiles each Gaussian touches (w * h of its rectangle)
    uint32_t* scan_blocks;    // [scan_nblocks(P, SCAN_ITEMS_PRE) + 64]: sized for the finer of the two scan granularities
    // Banded tile sort (binning.hip; per-tile path only, where depth_alt .. perm are free: no sub-buffers of their own)
    uint32_t* band_totals;    // [TILE_SORT_MAX_BANDS] instances per band of 256 tiles (scan_blocks_kernel); band bases = their prefix
    uint32_t* band_counts;    // [bands][scan_nblocks(P, SCAN_ITEMS_PRE)] instances of each 256-Gaussian scan block per band,
                              //     band-major; counted by preprocess, scanned along each band (exclusive, in place) by
                              //     scan_blocks_kernel
    uint32_t* band_live;      // [TILE_SORT_MAX_BANDS] pairs per band actually emitted (emit_banded_kernel: the totals, or with
                              //     fewer slots than instances what the kept slots hold); the segmented pass's band sizes
    size_t band_room;         // bytes from band_totals to the end of perm
    uint8_t* clamped;         // [P][4] SH colour clamp flags
    uint2* rect;              // [P] tile rectangle {x0 | y0 << 16, w | h << 16} (w = h = 0: culled), by Gaussian index; or
                              //     (ForwardPlan::rect_packed) uint32[2 P]: the first half x0 | y0 << 8 | w << 16 | h << 24,
                              //     which the depth sort carries along as a payload, the second half its ping-pong partner
    uint2* rect_sorted;       // [P] the same in depth order: written by the last pass of the depth sort, so that the
                              //     scan and duplicate read it coalesced instead of gathering through perm[]
    uint64_t* scan_status;    // [SCAN_SMALL_MAX_BLOCKS + 1] block totals of the single-launch scan + its ticket (zeroed by preprocess)
    uint32_t* tile_hist;      // [4][256] digit counts of the TILE sort's keys, counted by duplicate_kernel while it emits
                              //          them (zeroed by preprocess; lives here because the binning scratch only exists
                              //          once the instance count is known)
    void* sort_temp;          // depth sort scratch (directly behind tile_hist: preprocess clears all three in one sweep)
    size_t sort_temp_bytes;
    unsigned long long* prepare;   // [2] the backward accumulator whose gradient lines the NEXT blend forward clears, or 0:
                              //     [0] written by preprocess (mgs_forward_preprocess's prepare_backward), moved to [1] by
                              //     duplicate_kernel and read there by blend_forward_kernel -- one render call per hand-over
    char* end;                // one past the last carved byte
    static constexpr size_t ALIGN = 256;
    static size_t bytes(int P);
    static GeometryState carve(void* base, int P);
};
constexpr int SCAN_SMALL_MAX_BLOCKS = 64;     // up to this many scan blocks (P <= 131 072) the scan is ONE launch

struct ImageState {
    float* final_T;      // [H*W]
    uint32_t* n_contrib; // [H*W]
    uint2* ranges;       // [tiles]
    static constexpr size_t ALIGN = 256;
    static size_t bytes(int W, int H);
    static ImageState carve(void* base, int W, int H);
};

struct BinningState {
    uint32_t* keys_a;          // tile id per instance, emitted in (depth, index) order; sort input
    uint32_t* vals_a;
    uint32_t* keys_b;          // ping-pong partners
    uint32_t* vals_b;
    uint32_t* keys_sorted;     // = keys_a or keys_b: tile ids grouped by tile (stable)
    uint32_t* vals_sorted;     // = vals_a or vals_b: "point_list", Gaussian index per instance in blend order
    void* sort_temp;
    size_t sort_temp_bytes;
    uint32_t* count;           // [2] capacity mode: live instance count, overflow flag
    unsigned long long* fwd_masks;   // [R / 64 + tiles + 1][4] the blend forward's survivor masks, one word per (64-instance step,
                               //     quadrant): step b of a tile whose list starts at x has the row x / 64 + tile + b, which
                               //     no other tile's step has; written by blend_forward_kernel, walked by blend_backward_s_kernel
    static size_t fwd_mask_rows(uint64_t R, int W, int H);
    static constexpr size_t ALIGN = 256;
    static size_t bytes(uint64_t R, int W, int H);
    static BinningState carve(void* base, uint64_t R, int W, int H);
};

// Items per scan block.  The scan kernels of binning.hip take SCAN_ITEMS Gaussians per workgroup; on the per-tile path
// preprocess_forward_kernel scans its own 256 Gaussians (SCAN_ITEMS_PRE) and no scan_local launch follows.  Which one a
// forward uses: ForwardPlan::scan_items; it travels to the kernels as a shift.
constexpr int SCAN_ITEMS = 2048;
constexpr int SCAN_ITEMS_PRE = 256;      // = the workgroup of preprocess_forward_kernel
inline int scan_nblocks(int P, int items) { return (P + items - 1) / items; }

// Banded tile sort (binning.hip): on the per-tile path, when the tile id is wider than one 8-bit digit and the image has at
// most TILE_SORT_MAX_BANDS bands of 256 tiles, the instances are emitted already grouped by band (exact counts from
// preprocess) and ONE segmented 8-bit pass orders each band (ForwardPlan::bands_counted, ForwardPlan::bands).
constexpr int TILE_BAND_BITS = 8;
constexpr int TILE_SORT_MAX_BANDS = 32;
inline size_t band_table_bytes(int P, int bands) { return (64 + (size_t)bands * ((P + 255) / 256)) * sizeof(uint32_t); }

inline int tiles_x(int W) { return (W + TILE - 1) / TILE; }
inline int tiles_y(int H) { return (H + TILE - 1) / TILE; }
inline int tile_bits(int W, int H) {     // bits of the tile id that can be set
    uint32_t n = (uint32_t)(tiles_x(W) * tiles_y(H));
    int b = 0;
    while ((1u << b) < n && b < 31) ++b;
    return b == 0 ? 1 : b;
}

// Depth keys: float bits of a view-space depth > 0.2 (preprocess culls the rest; all ones = culled).  key - DEPTH_KEY_SUB
// stays below DEPTH_KEY_NARROW = 2^27 - 1 for every depth below 13 107.2 units (radix_sort.hip).
constexpr uint32_t DEPTH_KEY_SUB = 0x3E4CCCCDu;             // float bits of 0.2f
constexpr uint32_t DEPTH_KEY_NARROW = (1u << 27) - 1u;
// Per-tile depth order (binning.hip): the tile sort's key is tile << (32 - tb) | depth27 >> lo, its value
// (depth27 & (2^lo - 1)) << (32 - lo) | index, with depth27 = min(key - DEPTH_KEY_SUB, DEPTH_KEY_NARROW) and lo = the
// depth bits that do not fit beside a tile id of tb bits
__host__ __device__ inline int tile_depth_lo_bits(int tb) { return tb > 5 ? tb - 5 : 0; }

// the three scratches of a finished (or running) forward, carved together (api.hip)
struct ForwardStates { GeometryState g; ImageState img; BinningState b; };
ForwardStates carve_forward(const void* geometry, const void* binning, const void* image, int P, uint64_t R, int W, int H);

// ---- error plumbing --------------------------------------------------------------------------
void set_error(const char* fmt, ...);
#define MGS_HIP(expr)                                                                     \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            mgs::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return 2;                                                                     \
        }                                                                                 \
    } while (0)

// The first checks of an entry point that takes a camera and a map (api.hip); 1 with the error set.  `who`: the entry point's
// name, put in front of the text ("who: text"), or NULL for the bare text.  check_map_size: the blend backward forms
// `index * 64 + slot` in 32 bits (blend.hip, bt_flush), so a larger map is refused everywhere.
int check_cam(const mgs_camera* cam, const char* who = nullptr);
int check_map_size(int32_t P, const char* who = nullptr);

// ---- stage launchers (one per translation unit) ------------------------------------------
struct StageTimer;  // api.hip

int launch_preprocess_forward(const ForwardPlan& plan, const mgs_camera& cam, const float* means3D, const float* shs,
                              const float* colors_precomp, const float* opacities, const float* scales,
                              const float* rotations, const float* cov3D_precomp,
                              const GeometryState& g, int32_t* radii, float* prepare_grad_acc, hipStream_t s);
// backward scratch: the accumulator, then -- 64-byte lines like its own, so that one clear covers both -- the pose part
constexpr int TAU_SLOTS = 256;              // one 64-byte line each
struct BackwardState {
    float* grad_acc;     // [P][16] gradient lines
    float* tau_part;     // [TAU_SLOTS][16] pose-gradient slots
    float* tau;          // [16] dL/dtau of a prepared backward: floats 0..5 (rho, theta); 6..9 (dfx, dfy, dcx, dcy) with
                         //      MGS_FLAG_INTRINSICS_GRAD; the same lanes of every tau_part line
    static constexpr size_t ALIGN = 64;
    static size_t bytes(int P);
    static BackwardState carve(void* base, int P);
};
// `prepare_grad_acc` (or NULL): the pose part behind the accumulator is cleared by the kernel itself; the accumulator's address is
// left in g.prepare[0] for the render call that follows, whose blend forward clears the P gradient lines (blend.hip)
// (the scan runs over rect_sorted after a depth sort, over rect by index on the per-tile path)
int launch_scan(const ForwardPlan& plan, const GeometryState& g, hipStream_t s);
// `count` (device, capacity mode): [0] live instance count min(R, r_cap), [1] overflow flag
int launch_duplicate(const ForwardPlan& plan, const GeometryState& g, const BinningState& b, const ImageState& img,
                     int32_t* n_touched, uint32_t* count, uint32_t* overflow, hipStream_t s);
size_t sort_temp_bytes(uint64_t n, int bits);
size_t radix_temp_bytes(uint64_t n, int bits);
size_t radix_depth_temp_bytes(uint64_t n);
bool radix_result_in_b(int bits);
constexpr int RADIX_ERROR_WORDS = 4;      // = RS_MAX_PASSES (radix_sort.hip)
const uint32_t* radix_error_flag(void* temp, uint64_t n, int bits);
const uint32_t* radix_depth_error_flag(void* temp, uint64_t n);
__device__ __forceinline__ uint32_t radix_failed(const uint32_t* __restrict__ e) { return (e[0] | e[1]) | (e[2] | e[3]); }
void radix_zero_region(void* temp, uint64_t n, int bits, uint32_t** ptr, size_t* words);   // what must be 0 before a sort
void radix_depth_zero_region(void* temp, uint64_t n, uint32_t** ptr, size_t* words, bool header_only = false);
struct RadixSortOptions {
    const uint32_t* n_dev = nullptr;         // the live pair count is read on the device (min(n, *n_dev)); n is the capacity
    bool temp_zeroed = false;                // the caller cleared radix_zero_region()
    const uint2* aux_in = nullptr; uint2* aux_out = nullptr;     // last pass also writes aux_out[i] = aux_in[value i]
    bool aux_empty_for_ones = false;         // a key of all ones gets aux (0, 0) without the fetch
    const uint32_t* ext_hist = nullptr;      // [4][256], one-sweep path only (radix_size_class(n) != RADIX_COUNTED): digit counts of the keys,
                                             // counted by the kernel that produced them -- the sort launches no histogram kernel
    bool exclusive = false;                  // MGS_FLAG_EXCLUSIVE_DEVICE: small sorts may use block ids as tile ids
    uint2* ranges = nullptr;                 // keys are small integers: ranges[key] = {first, last + 1} sorted position
                                             // (the final pass: atomicMin / atomicMax on words preset to {~0, 0})
    int key_shift = 0;                       // the bits sorted are [key_shift, key_shift + bits); ranges are indexed
                                             // by key >> key_shift, and the final pass keeps the keys
};
int radix_sort_pairs(uint32_t* ka, uint32_t* va, uint32_t* kb, uint32_t* vb, uint64_t n, int bits, void* temp,
                     hipStream_t s, const RadixSortOptions& o);
// The size class of a sort of n pairs, for the forward plan.  RADIX_COUNTED: the counted-tiles path (a payload can travel, no global digit histogram
// is read).  RADIX_COUNTED_WANTED: the "radix_scanned" knob asks for it, n is too small to be forced onto it: one sweep, but a map that size counts as large.
enum RadixSizeClass { RADIX_ONE_SWEEP = 0, RADIX_COUNTED_WANTED = 1, RADIX_COUNTED = 2 };
RadixSizeClass radix_size_class(uint64_t n);
// Banded tile sort (radix_sort.hip): (ka, va) hold <= 32 independent runs end to end, run b of band_totals[b] pairs (device);
// ONE counted-tiles pass on key bits [key_shift, key_shift + 8) orders each run into the same positions of (kb, vb) and
// writes `ranges` (indexed by key >> key_shift).  Scratch: radix_banded_temp_bytes(n, bands), its zero region as for the other sorts.
size_t radix_banded_temp_bytes(uint64_t n, int bands);
void radix_banded_zero_region(void* temp, uint64_t n, int bands, uint32_t** ptr, size_t* words);
int radix_sort_banded(const uint32_t* ka, const uint32_t* va, uint32_t* kb, uint32_t* vb, uint64_t n, int key_shift, void* temp,
                      hipStream_t s, const uint32_t* n_dev, const uint32_t* band_totals, int bands, uint2* ranges);
// The forward's first sort (radix_sort.hip): depth keys -> perm + rect_sorted; three 9-bit passes (+ a fourth that only
// runs for depths beyond 13 107 units).  `payload` (ForwardPlan::rect_packed): the sort carries the packed rectangles itself.
int radix_sort_depth(uint32_t* keys, uint32_t* key_b, uint32_t* val_a, uint32_t* val_b, void* rect, bool payload,
                     uint32_t* perm, uint2* rect_sorted, uint64_t n, void* temp, hipStream_t s, bool temp_zeroed,
                     bool exclusive = false);
int launch_depth_sort(const ForwardPlan& plan, const GeometryState& g, hipStream_t s);
// `n_dev`: capacity mode's live pair count (NULL: plan.R); the final pass writes img.ranges
int launch_sort(const ForwardPlan& plan, const GeometryState& g, const BinningState& b, const ImageState& img,
                const uint32_t* n_dev, hipStream_t s);
// per-tile depth order: each tile's list, grouped by the tile sort in index order, sorted by (depth, index) in place
// (tile_sort.h) -- by blend_forward_kernel (ForwardPlan::tile_sort_fused) or by a launch of its own
struct TileSortArgs {
    uint32_t* keys;                            // the tile sort's output pairs: read, and the long-list path's ping-pong
    uint32_t* vals;                            // = point_list: the sorted indices are written here in place
    uint32_t* keys_alt;
    uint32_t* vals_alt;
    const uint32_t* depth_key;
    const uint32_t* n_dev;                     // capacity mode: live pair count (NULL: n_cap)
    uint32_t n_cap;
    int tb;                                    // tile bits
};
TileSortArgs tile_sort_args(const ForwardPlan& plan, const GeometryState& g, const BinningState& b, const uint32_t* n_dev);
int launch_tile_depth_sort(const ForwardPlan& plan, const TileSortArgs& ts, const ImageState& img, const uint32_t* sort_err,
                           hipStream_t s);
int set_radix_spin_limit(uint32_t limit);
extern bool g_opt_blend_bwd_transposed_set;
extern int g_dbg_last_bwd_split, g_dbg_last_tile_sort_bands;
extern int g_opt_radix_ballot_rank, g_opt_radix_scanned, g_opt_radix_xcd_band, g_opt_knn_grid_min, g_opt_scan_small, g_opt_pre_scan, g_opt_tile_sort_banded, g_opt_tile_sort_fused, g_opt_dup_slot_major, g_opt_blend_bwd_transposed, g_opt_blend_bwd_split, g_opt_blend_bwd_split_min, g_opt_blend_bwd_split_frac;      // test knobs (mgs_debug_set_option)
// `sort_err`: the tile sort's error words (NULL: nothing was sorted); a raised word empties every tile and sets
// MGS_STATUS_TILE_SORT_TIMEOUT in *status (what ranges_kernel did until round 4).  `ts`: read with plan.tile_sort_fused, when
// every workgroup first sorts its tile's list (tile_sort.h)
int launch_blend_forward(const ForwardPlan& plan, const mgs_camera& cam, const GeometryState& g, const BinningState& b,
                         const ImageState& img, float* out_color, float* out_depth, float* out_opacity,
                         int32_t* n_touched, const uint32_t* sort_err, uint32_t* status, const TileSortArgs& ts, hipStream_t s);
int launch_blend_backward(const mgs_camera& cam, const GeometryState& g, const BinningState& b,
                          const ImageState& img, const float* dL_dcolor, const float* dL_ddepth, const float* out_color,
                          const float* out_depth, float* grad_acc, bool pose_only, uint64_t num_rendered, hipStream_t s);
int launch_blend_backward_stats(const mgs_camera& cam, const GeometryState& g, const BinningState& b,
                                const ImageState& img, unsigned long long* stats, hipStream_t s);
int launch_blend_mask_stats(const mgs_camera& cam, const GeometryState& g, const BinningState& b,
                            const ImageState& img, unsigned long long* stats, hipStream_t s);
int launch_valu_ceiling(float* out, int iters, hipStream_t s);
// K feature channels through the tables of a finished forward (features.hip): read-only on all three scratch states
int launch_features_forward(const mgs_camera& cam, int P, int K, const GeometryState& g, const BinningState& b,
                            const ImageState& img, const float* features, const float* bg, float* out, int32_t* labels,
                            float min_opacity, hipStream_t s);
int launch_features_backward(const mgs_camera& cam, int P, int K, const GeometryState& g, const BinningState& b,
                             const ImageState& img, const float* dL_dout, float* dL_dfeatures, hipStream_t s);
// the headless viewer (viewer.hip): the ellipsoid walk reads the three scratch states, lines and compose share `scratch`
int launch_viewer_ellipsoids(const mgs_camera& cam, int P, const GeometryState& g, const BinningState& b, const ImageState& img,
                             float threshold, float* out, int32_t* hit, hipStream_t s);
size_t viewer_scratch_bytes(int W, int H);
int launch_viewer_lines(int W, int H, const int32_t* segs, int S, void* scratch, hipStream_t s);
int launch_viewer_compose(int mode, int W, int H, const float* src, const uint8_t* lut, const uint8_t* seg_rgb, int S,
                          void* scratch, uint8_t* out, hipStream_t s);
struct GeomBackwardArgs {
    const float *means3D, *shs, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp;
    const int32_t* radii;
    const float* grad_acc;   // [P][16] from the blend backward
    float *dL_dmeans2D, *dL_dcolors, *dL_dopacity, *dL_dmeans3D, *dL_dcov3D, *dL_dsh, *dL_dscales,
        *dL_drotations, *dL_dtau;
    float* tau_part;         // [TAU_SLOTS][16] zeroed partial pose gradients (large launches), or NULL: add into dL_dtau directly
};
constexpr int TAU_DIRECT_MAX_BLOCKS = 256;  // up to this many workgroups the direct same-address adds are cheaper than a launch
int launch_geom_backward(const mgs_camera& cam, int P, const GeometryState& g, const GeomBackwardArgs& a,
                         hipStream_t s);
int launch_mark_visible(int P, const float* means3D, const float* viewmatrix, uint8_t* visible, hipStream_t s);
size_t knn_scratch_bytes(int P);
int launch_knn(int P, const float* points, float* out, void* scratch, hipStream_t s);

// ---- the Morton-box index of a point set (knn.hip), built for mgs_dist2_knn and for mgs_nn_dist2 (mesheval.hip) ----
// the ONE pair formula of every nearest-neighbour path (explicit fma chain so that all of them compile to the same three instructions)
__device__ __forceinline__ float pair_d2(float cx, float cy, float cz, float qx, float qy, float qz) {
    const float dx = cx - qx, dy = cy - qy, dz = cz - qz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
struct MortonIndex {
    int32_t* bbox;            // [8] ordered-int min xyz (0..2), max xyz (4..6)
    uint32_t *code_a, *code_b, *idx_a, *idx_b;
    float4* sorted;           // [P] x, y, z, bits(original index), Morton order
    float4* box_lo;           // [ceil(P / 64)] bounds of 64 consecutive sorted points
    float4* box_hi;
    void* sort_temp;
    size_t bytes;
};
MortonIndex morton_carve(void* base, int P);
void morton_bbox_reset(int32_t* bbox, hipStream_t s);                               // an empty box
void morton_bbox_extend(int P, const float* points, int32_t* bbox, hipStream_t s);  // bbox |= points (integer atomics: exact)
// 30-bit codes inside `bbox` (any device box that holds the points), the radix sort, `sorted` + box bounds.  `codes_sorted`: where
// the sorted codes lie (one of k.code_a / k.code_b)
int morton_build(int P, const float* points, const int32_t* bbox, const MortonIndex& k, hipStream_t s,
                 const uint32_t** codes_sorted = nullptr);
constexpr int KNN_BOX = 64;                 // points per Morton box = one wave of queries
constexpr int KNN_GRID_MIN = 6144;          // below this many points the all-pairs sweep wins (no sort, no index).  Measured, round 2:
                                            // 4 k points 0.147 vs 0.207 ms, 8 k 0.291 vs 0.246, 16 k 0.58 vs 0.33, 32 k 1.17 vs 0.36 ms
constexpr float KNN_FLT_MAX = 3.402823466e+38f;
// float <-> int whose signed order is the float order (for atomicMin / atomicMax)
__device__ __forceinline__ int32_t f2ord(float f) { const int32_t i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7FFFFFFF; }
__device__ __forceinline__ float ord2f(int32_t i) { return __int_as_float(i >= 0 ? i : i ^ 0x7FFFFFFF); }
__device__ __forceinline__ float gap(float lo, float hi, float qlo, float qhi) {   // distance between [lo,hi] and [qlo,qhi]
    return fmaxf(0.f, fmaxf(lo - qhi, qlo - hi));
}

// The walk over the boxes of a Morton index by ONE WAVE for its 64 queries (lane: query q, `live` or a copy of the last one; the
// wave's own bounds qlo / qhi; `cand[wv]`: the 64 float4 of LDS that belong to the wave).  A box is staged there between two wave
// barriers and swept by all lanes as broadcasts.  The boxes are pruned 64 at a time (lane l: box base + l) against the wave's
// bounds and the largest bound of its lanes, each survivor is re-checked per lane, swept if any lane needs it, and the wave's
// maximum refreshed.  The lower bound of a box is the pair formula applied to coordinate gaps that rounding can only shrink
// (c >= lo => fl(c - q) >= fl(lo - q), squares and fmas are monotone); the 0.99999 is an extra margin.  What differs between
// the users is the policy:
//   void take(const float4& c, const float4& q, int i, int b)    candidate i of box b against the lane's running result
//   float bound() const                             the distance beyond which the lane has no use for a candidate
//   static bool keep(float lower, float bound)      may a box (or lane) with this lower bound still matter?
//   int seed(sweep)                                 sweeps a box and its two neighbours along the curve, returns the middle one
//   void store(const float4& q) const               writes a live lane's result (inside the walk: behind it, the compiler lays the
//                                                   loop's exit out differently from the kernels this was lifted from)
template <typename Policy>
__device__ __forceinline__ void morton_box_walk(Policy& pol, int P, int nb, const float4* sorted, const float4* box_lo,
                                                const float4* box_hi, const float4& q, const float4& qlo, const float4& qhi,
                                                bool live, int lane, float4 (*cand)[KNN_BOX], int wv) {
    auto sweep = [&](int b) {                   // all 64 lanes against the (<= 64) points of box b
        const int ci = b * KNN_BOX + lane;
        __builtin_amdgcn_wave_barrier();
        cand[wv][lane] = ci < P ? sorted[ci] : make_float4(KNN_FLT_MAX, KNN_FLT_MAX, KNN_FLT_MAX, 0.f);
        __builtin_amdgcn_wave_barrier();
        const int n = min(KNN_BOX, P - b * KNN_BOX);
        for (int i = 0; i < n; ++i) {
            const float4 c = cand[wv][i];
            pol.take(c, q, i, b);
        }
    };
    const int sb = pol.seed(sweep);
    float wmax = wave_max(live ? pol.bound() : 0.f);     // no lane of the wave can still use a box farther than this
    for (int base = 0; base < nb; base += 64) {
        const int bi = base + lane;
        bool want = bi < nb && (bi < sb - 1 || bi > sb + 1);
        if (want) {
            const float4 lo = box_lo[bi], hi = box_hi[bi];
            const float gx = gap(lo.x, hi.x, qlo.x, qhi.x), gy = gap(lo.y, hi.y, qlo.y, qhi.y), gz = gap(lo.z, hi.z, qlo.z, qhi.z);
            want = Policy::keep(fmaf(gz, gz, fmaf(gy, gy, gx * gx)) * 0.99999f, wmax);
        }
        unsigned long long mask = __builtin_amdgcn_ballot_w64(want);
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int b = base + j;                                  // wave-uniform
            const float4 lo = box_lo[b], hi = box_hi[b];
            const float gx = gap(lo.x, hi.x, q.x, q.x), gy = gap(lo.y, hi.y, q.y, q.y), gz = gap(lo.z, hi.z, q.z, q.z);
            const bool need = live && Policy::keep(fmaf(gz, gz, fmaf(gy, gy, gx * gx)) * 0.99999f, pol.bound());
            if (__builtin_amdgcn_ballot_w64(need) == 0ull) continue;
            sweep(b);
            wmax = wave_max(live ? pol.bound() : 0.f);
        }
    }
    if (live) pol.store(q);
}

}  // namespace mgs
