// Binning: depth order of the Gaussians, prefix sum of tiles touched, duplicate-with-tile-ids,
// stable grouping by tile, per-tile ranges.
//
// Boundary replaced: upstream cub::DeviceScan::InclusiveSum, duplicateWithKeys,
// cub::DeviceRadixSort::SortPairs and identifyTileRanges.
// Integer work; the per-tile lists are bit-exact with the upstream definition
//   order inside a tile = ascending (float32 bits of the view-space depth, Gaussian index)
// but they are produced with far less sort traffic than one 64-bit (tile | depth) sort of all R
// instances:  (1) stable sort of the P Gaussians by their 32 depth bits (ties keep index order),
// (2) instances emitted in that order, (3) stable sort of the R instances on the tile id only
// (13 bits at 1080p: 2 radix passes over 8-byte pairs instead of 6 passes over 12-byte pairs).
// Stability of both sorts makes the result identical to the single 64-bit sort.  The sort itself is
// the hand-written LSD radix sort of radix_sort.hip.  The last pass of the depth sort also lays the tile
// rectangles out in depth order, so the scan and duplicate below read everything coalesced.
//
// Large maps (ForwardPlan::per_tile) skip (1): the instances are emitted in index order with their depth in the pair and each
// tile's list is sorted by depth on its own (tile_sort.h).  There the tile sort only has to group by tile, stably -- and the
// band of 256 tiles an instance falls into is known where the instance is made: ForwardPlan::bands != 0 emits the instances
// grouped by band from exact counts (preprocess counts them per scan block, scan_blocks_kernel scans them, emit_banded_kernel
// places them) and (3) is ONE segmented 8-bit pass, radix_sort_banded, instead of two passes over everything.
#include "common.h"
#include "tile_sort.h"


namespace mgs {

// ------------------------------------------------------------------------------------------------
// inclusive scan of uint32 in two steps: per-block local scan + block sums, exclusive scan of the block sums
// (+ the grand total).  Global offset of element i = local[i] + block_sums[i / items], items = ForwardPlan::scan_items:
//   SCAN_ITEMS (2048; 256 threads x 8 items): scan_local_kernel, a launch of its own over the rectangles -- the global path,
//     where the scan runs in depth order, after the depth sort;
//   SCAN_ITEMS_PRE (256): the per-tile path, where the scan runs in index order: preprocess_forward_kernel has the
//     rectangles in registers and scans its own workgroup's (preprocess.hip); only scan_blocks_kernel is launched.
// The consumers (duplicate_kernel) take the granularity as a shift.
// ------------------------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 256;
__device__ __forceinline__ int scan_nblocks_dev(int P, int shift) { return (P + (1 << shift) - 1) >> shift; }
constexpr int SCAN_PER_THREAD = SCAN_ITEMS / SCAN_THREADS;

// Items of a scan block are dealt out wave by wave, row by row: wave w owns items [w * 512, (w + 1) * 512) of the block, item
// (i, lane) = i * 64 + lane of them -- every load and every store of a wave is 64 consecutive elements.  (The first version
// gave a thread 8 CONSECUTIVE items: each of its 8 loads / stores touched all 64 lines of the wave's span an eighth each,
// the shape that cost the per-Gaussian forward 30 us at C5.)  Row i of a wave is scanned with the DPP wave scan and
// offset by the rows before it; the waves are joined through LDS.  Returns the block-wide total; incl[i] = inclusive sum up
// to item (i, lane) within the block.
__device__ __forceinline__ uint32_t scan_block_rows(const uint2* __restrict__ rects, int n, int cbase, int lane, int wv,
                                                    uint32_t (&incl)[SCAN_PER_THREAD], uint32_t* smem /* >= 4 */) {
    uint32_t v[SCAN_PER_THREAD];
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) {
        const int idx = cbase + i * WAVE + lane;
        const uint32_t wh = idx < n ? rects[idx].y : 0u;                   // tiles touched = w * h of the rectangle
        v[i] = (wh & 0xFFFFu) * (wh >> 16);
    }
    uint32_t run = 0;                                                      // wave-uniform: rows before this one
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) {
        const uint32_t sc = wave_incl_scan_dpp(v[i]);
        incl[i] = run + sc;
        run += (uint32_t)__builtin_amdgcn_readlane((int)sc, 63);
    }
    if (lane == 0) smem[wv] = run;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wv; ++w) wbase += smem[w];
    const uint32_t total = (smem[0] + smem[1]) + (smem[2] + smem[3]);
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) incl[i] += wbase;
    return total;
}

// out[i] = inclusive sum of the tiles touched by the Gaussians j <= i in depth order (rects = rect_sorted), within the block
// (per-tile depth order: in index order, rects = rect)
__global__ void __launch_bounds__(SCAN_THREADS) scan_local_kernel(const uint2* __restrict__ rects, uint32_t* out,
                                                                  uint32_t* block_sums, int n) {
    __shared__ uint32_t smem[8];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cbase = blockIdx.x * SCAN_ITEMS + wv * (SCAN_PER_THREAD * WAVE);
    uint32_t incl[SCAN_PER_THREAD];
    const uint32_t total = scan_block_rows(rects, n, cbase, lane, wv, incl, smem);
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) {
        const int idx = cbase + i * WAVE + lane;
        if (idx < n) out[idx] = incl[i];
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// single workgroup: exclusive scan of the block sums in place.  1024 threads x 8 items: the 7 813 sums of 256 Gaussians each
// at C5 are ONE iteration (256 threads x 1 item took 31 dependent ones); larger maps loop.  Items are dealt out as in
// scan_block_rows: wave w owns items [w * 512, (w + 1) * 512) of the iteration, item (i, lane) = i * 64 + lane of them.
constexpr int SCANB_THREADS = 1024, SCANB_PER_THREAD = 8, SCANB_WAVES = SCANB_THREADS / WAVE;
constexpr int SCANB_ITEMS = SCANB_THREADS * SCANB_PER_THREAD;
// Banded tile sort: the launch has one more workgroup per band; workgroup 1 + b scans row b of band_counts (the column of
// band b over the scan blocks) the same way and leaves the band's total in band_totals[b].  Nobody waits for anybody.
__global__ void __launch_bounds__(SCANB_THREADS) scan_blocks_kernel(uint32_t* block_sums, int nblocks, uint32_t* band_counts,
                                                                    uint32_t* band_totals) {
    __shared__ uint32_t smem[SCANB_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t* total_out = block_sums + nblocks;             // grand total = number of instances R (read back by the exact path)
    if (blockIdx.x > 0) {                                   // (workgroup-uniform)
        block_sums = band_counts + (size_t)(blockIdx.x - 1) * nblocks;
        total_out = band_totals + (blockIdx.x - 1);
    }
    uint32_t carry = 0;
    for (int start = 0; start < nblocks; start += SCANB_ITEMS) {          // (workgroup-uniform: every thread reaches the barriers)
        const int cbase = start + wv * (SCANB_PER_THREAD * WAVE);
        uint32_t v[SCANB_PER_THREAD], incl[SCANB_PER_THREAD];
#pragma unroll
        for (int i = 0; i < SCANB_PER_THREAD; ++i) {
            const int idx = cbase + i * WAVE + lane;
            v[i] = idx < nblocks ? block_sums[idx] : 0u;
        }
        uint32_t run = 0;                                                  // wave-uniform: rows before this one
#pragma unroll
        for (int i = 0; i < SCANB_PER_THREAD; ++i) {
            const uint32_t sc = wave_incl_scan_dpp(v[i]);
            incl[i] = run + sc;
            run += (uint32_t)__builtin_amdgcn_readlane((int)sc, 63);
        }
        if (lane == 0) smem[wv] = run;
        __syncthreads();
        uint32_t wbase = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SCANB_WAVES; ++w) {
            const uint32_t t = smem[w];
            wbase += w < wv ? t : 0u;
            total += t;
        }
#pragma unroll
        for (int i = 0; i < SCANB_PER_THREAD; ++i) {
            const int idx = cbase + i * WAVE + lane;
            if (idx < nblocks) block_sums[idx] = carry + wbase + incl[i] - v[i];
        }
        carry += total;
        __syncthreads();                                                   // smem is rewritten by the next iteration
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// ONE launch for P <= SCAN_SMALL_MAX_BLOCKS * SCAN_ITEMS (every SLAM-sized map): each workgroup publishes its total as a
// self-describing 8-byte word {1 << 63 | total} (one relaxed agent-scope store, polled with relaxed agent-scope loads:
// the radix sort's protocol), lane j of its first wave waits for block j < its own, the wave adds them up.  Which block
// of the input a workgroup takes is decided by an atomic ticket (status[SCAN_SMALL_MAX_BLOCKS], zeroed with the status
// words), as in the radix sort: a workgroup then only ever waits for workgroups that have already started, whatever
// else shares the device.  Under MGS_FLAG_EXCLUSIVE_DEVICE the <= 64 workgroups are co-resident (one per CU) and the
// block id serves.  The spin is bounded anyway and raises the depth sort's error word (the consumers of the scan are
// the consumers of that sort).  out[] then holds GLOBAL inclusive sums; the grand total goes to block_sums[nblocks].
constexpr uint32_t SCAN_SPIN_LIMIT = 1u << 22;
__global__ void __launch_bounds__(SCAN_THREADS) scan_small_kernel(const uint2* __restrict__ rects, uint32_t* out,
                                                                  uint32_t* block_sums, uint64_t* status, int n, int nb,
                                                                  uint32_t* err, int ticketed) {
    __shared__ uint32_t smem[8];
    __shared__ uint32_t s_prefix, s_bid;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int bid = (int)blockIdx.x;
    if (ticketed) {
        if (threadIdx.x == 0) s_bid = atomicAdd((uint32_t*)(status + SCAN_SMALL_MAX_BLOCKS), 1u);
        __syncthreads();
        bid = (int)s_bid;
    }
    const int cbase = bid * SCAN_ITEMS + wv * (SCAN_PER_THREAD * WAVE);
    uint32_t incl[SCAN_PER_THREAD];
    const uint32_t total = scan_block_rows(rects, n, cbase, lane, wv, incl, smem);
    if (threadIdx.x == 0)
        __hip_atomic_store(status + bid, (1ull << 63) | (uint64_t)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x < WAVE) {
        uint32_t before = 0;
        if ((int)threadIdx.x < bid) {
            uint64_t w = 0;
            uint32_t spins = 0;
            while (true) {
                w = __hip_atomic_load(status + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (w >> 63) break;
                if (++spins > SCAN_SPIN_LIMIT) { atomicExch(err, 1u); break; }
                __builtin_amdgcn_s_sleep(1);
            }
            before = (uint32_t)w;
        }
        MGS_WAVE_REDUCE(before, MGS_WAVE_ADD);
        if (threadIdx.x == 0) s_prefix = before;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) {
        const int idx = cbase + i * WAVE + lane;
        if (idx < n) out[idx] = incl[i] + s_prefix;
    }
    if (threadIdx.x == 0 && bid == nb - 1) block_sums[nb] = s_prefix + total;
}

// ---- The forward plan (forward_plan.h; DESIGN.md, "The forward plan"): every route decision of one forward, each rule written
// once, here.  Every launcher reads the plan; nothing outside this builder reads the five options below.
int g_opt_scan_small = -1;          // mgs_debug_set_option("scan_small", -1 | 0 | 1): 0 = always the two-launch scan
int g_opt_pre_scan = -1;            // mgs_debug_set_option("pre_scan", -1 | 0 | 1): 0 = per-tile path scans with launches of its own
int g_opt_tile_sort_banded = 1;     // mgs_debug_set_option("tile_sort_banded", 0): today's two tile-sort passes everywhere
int g_opt_dup_slot_major = -1;      // mgs_debug_set_option("dup_slot_major", -1 | 0 | 1): -1 = by size
int g_opt_tile_sort_fused = 1;      // mgs_debug_set_option("tile_sort_fused", 0): the per-tile depth sort as a launch of its own
int g_dbg_last_tile_sort_bands = 0; // mgs_debug_last_tile_sort_bands(): bands of the last emission launched (0: two passes)
constexpr uint64_t DUP_SLOT_MAJOR_MIN = 768ull * 1024;      // instances (capacity in capacity mode)
static_assert(SCAN_ITEMS == 1 << 11 && SCAN_ITEMS_PRE == 1 << 8, "scan_shift");

ForwardPlan forward_plan(int P, int W, int H, int flags) {
    ForwardPlan p{};
    p.P = P; p.W = W; p.H = H; p.flags = flags;
    p.tiles_x = tiles_x(W); p.tiles_y = tiles_y(H); p.ntiles = p.tiles_x * p.tiles_y;
    p.tile_bits = tile_bits(W, H); p.small_grid = p.ntiles <= 65536;
    // Depth order per tile (tile_depth_sort) wherever the map's depth sort would take the counted-tiles path -- or at any size
    // when the radix_scanned knob is 1 -- and the tile sort's keys have room for the high depth bits beside a tile id of
    // <= 16 bits, the values for the low ones beside the index: P <= 2^(37 - tile bits).  Else the global depth sort (one
    // sweep, or counted tiles with the knob at 0).
    const RadixSizeClass map_class = P > 0 ? radix_size_class((uint64_t)P) : RADIX_ONE_SWEEP;
    p.per_tile = map_class != RADIX_ONE_SWEEP && p.tile_bits <= 16 &&
                 (uint64_t)P <= (1ull << (32 - tile_depth_lo_bits(p.tile_bits)));
    // the scan's granularity: preprocess scans its own 256 Gaussians on the per-tile path (option "pre_scan" not 0)
    p.scan_items = (g_opt_pre_scan != 0 && p.per_tile) ? SCAN_ITEMS_PRE : SCAN_ITEMS;
    p.scan_shift = p.scan_items == SCAN_ITEMS_PRE ? 8 : 11; p.scan_blocks = scan_nblocks(P, p.scan_items);
    // (SCAN_ITEMS granularity only: the single-launch scan writes GLOBAL sums)
    p.scan_small = P > 0 && p.scan_items == SCAN_ITEMS && g_opt_scan_small != 0 && p.scan_blocks <= SCAN_SMALL_MAX_BLOCKS;
    // banded tile sort: the per-tile path where preprocess scans, a tile id wider than one digit, at most 32 bands of 256 tiles
    const int bands = (p.ntiles + (1 << TILE_BAND_BITS) - 1) >> TILE_BAND_BITS;
    p.bands_counted = (g_opt_tile_sort_banded != 0 && p.scan_items == SCAN_ITEMS_PRE && p.tile_bits > TILE_BAND_BITS &&
                       bands <= TILE_SORT_MAX_BANDS) ? bands : 0;
    // the depth sort carries the rectangles itself on its counted-tiles path; the packed form needs both grid dimensions in a byte
    p.rect_packed = !p.per_tile && map_class == RADIX_COUNTED && p.tiles_x <= 255 && p.tiles_y <= 255;
    p.exclusive = (flags & MGS_FLAG_EXCLUSIVE_DEVICE) != 0;
    return p;
}

ForwardPlan ForwardPlan::render(uint64_t R_in, bool capacity) const {
    ForwardPlan p = *this;
    p.capacity_mode = capacity;
    // No Gaussians: nothing was preprocessed, so nothing may be sorted whatever capacity the caller passed (background only)
    p.R = P == 0 ? 0 : R_in;
    p.r_cap = capacity ? (uint32_t)(p.R > 0xFFFFFFFFull ? 0xFFFFFFFFull : p.R) : (p.R > 0 ? 0xFFFFFFFFu : 0u);
    // Many instances AND many instances per Gaussian (big splats: the near ones cover hundreds of tiles), or forced: emission
    // balanced by output slots (see duplicate_kernel), with enough waves for ~512 slots each.  Otherwise the Gaussian-major
    // walk: no search, fewer loads per slot (C5, 2.6 instances per Gaussian: 22 us against 31 us slot-major; 102 k Gaussians at
    // 1200x680, 13 per Gaussian: 81 us against 8.6 us; 39 k at VGA, 415 k instances: 7.5 against 8.8 us).
    p.slot_major = P > 0 && g_opt_dup_slot_major != 0 &&
                   (g_opt_dup_slot_major > 0 || (p.R >= DUP_SLOT_MAJOR_MIN && p.R >= 6ull * (uint64_t)P));
    int n = P > ntiles ? P : ntiles;
    if (p.slot_major && p.R / 8 > (uint64_t)n) n = (int)(p.R / 8 > 0x3FFFFFFFull ? 0x3FFFFFFFull : p.R / 8);
    p.dup_threads = (n + 255) / 256 * 256;
    // The banded emission, once R is known.  Scenes of big splats keep the slot-balanced duplicate_kernel and the two passes:
    // emit_banded_kernel is one workgroup per 256 Gaussians, the Gaussian-major balance that kernel was built to escape (a
    // forced "dup_slot_major" = 1 is honoured the same way).  And the scratch of the one segmented pass must fit what
    // mgs_binning_bytes() reserves for the two passes (for a few thousand instances it does not: a partial tile per band
    // outweighs them).  0: the plain emission and the two passes, whatever preprocess counted.
    p.bands = (bands_counted && p.R > 0 && !p.slot_major &&
               radix_banded_temp_bytes(p.R, bands_counted) <= radix_temp_bytes(p.R, tile_bits)) ? bands_counted : 0;
    // duplicate_kernel counts the digits of the keys it emits where the tile sort reads a global histogram (one sweep)
    p.count_digits = !p.bands && P > 0 && tile_bits <= 16 && p.R > 0 && radix_size_class(p.R) != RADIX_COUNTED;
    p.key_shift = per_tile ? 32 - tile_bits : 0; p.depth_lo_bits = per_tile ? tile_depth_lo_bits(tile_bits) : 0;
    p.sort_tiles = per_tile && p.R > 0;
    p.tile_sort_fused = p.sort_tiles && g_opt_tile_sort_fused != 0;
    return p;
}


// (There is no third "add the block offset" pass: the only consumer of the offsets, duplicate_kernel, adds
//  block_sums[i / items] itself -- one launch and a 16-byte-per-Gaussian read-modify-write less.)

// (Measured and rejected: a single-workgroup scan for small P -- 1024 threads x a serial run of dependent
//  gathers each -- took ~300 us at P = 38 k against ~15 us for the three launches below: latency, not launches.)
//
// What is launched:  scan_items == SCAN_ITEMS_PRE (per-tile path): preprocess_forward_kernel already wrote the block-local sums
// of its 256-Gaussian workgroups and their totals -- scan_blocks_kernel alone, with a workgroup per counted band.
// scan_items == SCAN_ITEMS: scan_small_kernel (one launch, P <= 131 072) or scan_local_kernel + scan_blocks_kernel.
int launch_scan(const ForwardPlan& plan, const GeometryState& g, hipStream_t s) {
    const int P = plan.P, nb = plan.scan_blocks;
    if (P == 0) return 0;
    if (plan.scan_items == SCAN_ITEMS_PRE) {
        hipLaunchKernelGGL(scan_blocks_kernel, dim3(1 + plan.bands_counted), dim3(SCANB_THREADS), 0, s, g.scan_blocks, nb,
                           g.band_counts, g.band_totals);
        MGS_HIP(hipGetLastError());
        return 0;
    }
    // the rectangles in the order the scan runs in: depth order behind the depth sort, by index on the per-tile path
    const uint2* rects = plan.per_tile ? g.rect : g.rect_sorted;
    if (plan.scan_small) {
        hipLaunchKernelGGL(scan_small_kernel, dim3(nb), dim3(SCAN_THREADS), 0, s, rects, g.point_offsets, g.scan_blocks,
                           g.scan_status, P, nb, const_cast<uint32_t*>(radix_depth_error_flag(g.sort_temp, (uint64_t)P)),
                           plan.exclusive ? 0 : 1);
        MGS_HIP(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(scan_local_kernel, dim3(nb), dim3(SCAN_THREADS), 0, s, rects, g.point_offsets,
                       g.scan_blocks, P);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(SCANB_THREADS), 0, s, g.scan_blocks, nb, nullptr, nullptr);
    MGS_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// duplicate: thread i takes the i-th Gaussian in depth order and walks its tile rectangle
// (y outer, x inner), emitting (tile id, Gaussian index)
//
// Per-tile depth order (`depth_key` non-NULL, perm NULL): the i-th Gaussian by INDEX, and the pair carries its depth --
// key = tile << tshift | depth27 >> lo, value = (depth27 & (2^lo - 1)) << (32 - lo) | index (common.h).  Depths beyond
// the narrow range are clamped to DEPTH_KEY_NARROW; tile_depth_sort_kernel re-sorts that trailing run by the full key.
// ------------------------------------------------------------------------------------------------
// (`k`: depth_key[gidx], loaded by the caller beside its other inputs; `keyed`: there is a depth key)
__device__ __forceinline__ void dup_pair(uint32_t gidx, bool keyed, uint32_t k, int lo, uint32_t& val, uint32_t& kfield) {
    val = gidx; kfield = 0u;
    if (keyed) {
        const uint32_t d = k == 0xFFFFFFFFu ? DEPTH_KEY_NARROW : min(k - DEPTH_KEY_SUB, DEPTH_KEY_NARROW);
        kfield = d >> lo;
        if (lo) val |= (d & ((1u << lo) - 1u)) << (32 - lo);
    }
}
// Slot t of a rectangle w tiles wide -> (row, column) = (t / w, t % w).  t < 65 536 (`small`: the grid has at most 2^16
// tiles -- always on the per-tile path), so t and w are exact in float32 and one multiply by a reciprocal rounded DOWN gives
// the quotient or one less: v_rcp_f32 is good to 1 ulp, two ulps are taken off, so r <= 1 / w and t * r <= t / w
// <= q + 1 - 1 / w; the product's rounding error is below q * 2^-24 < 1 / w, so it stays below q + 1, and from below it loses
// less than 65 536 * 5 * 2^-24 < 1.  One correction step settles it (tests/test_dup_slot_decode.py runs the formula over every
// t < 65 536, w <= 4 096 and every reciprocal 1 ulp around the exact one).  A full 32-bit division is ~40 instructions per
// emitted slot; larger grids keep it.
__device__ __forceinline__ void dup_divmod(uint32_t t, uint32_t w, bool small, uint32_t& q, uint32_t& rem) {
    if (small) {
        const float r = __uint_as_float(__float_as_uint(__builtin_amdgcn_rcpf((float)w)) - 2u);
        q = (uint32_t)((float)t * r);
        rem = t - q * w;
        if (rem >= w) { q += 1u; rem -= w; }
    } else {
        q = t / w; rem = t - q * w;
    }
}
// What a lane needs of the Gaussian that owns its slot, as ONE 16-byte LDS entry (a ds_read_b128; six 4-byte gathers
// before) + the key field: {first slot, tile id of the rectangle's corner, width, value of the pair}
__device__ __forceinline__ uint4 dup_entry(uint32_t first, int x0, int y0, int w, int gx, uint32_t val) {
    return make_uint4(first, (uint32_t)(y0 * gx + x0), (uint32_t)max(w, 1), val);
}
__device__ __forceinline__ void dup_emit(const uint4 e, uint32_t kf, uint32_t o, int gx, int tshift, bool small,
                                         uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t& key) {
    uint32_t yy, xx;
    dup_divmod(o - e.x, e.z, small, yy, xx);
    const uint32_t tid = e.y + yy * (uint32_t)gx + xx;
    key = (tid << tshift) | kf;
    keys[o] = key;
    vals[o] = e.w;
}
__global__ void __launch_bounds__(256) duplicate_kernel(int P, const uint2* __restrict__ rects,
                                                        const uint32_t* __restrict__ perm,
                                                        const uint32_t* __restrict__ depth_key, int tshift, int lo,
                                                        const uint32_t* __restrict__ offsets /* block-local inclusive sums */,
                                                        const uint32_t* __restrict__ block_sums /* [nb] exclusive, [nb] = total */,
                                                        uint32_t* keys,
                                                        uint32_t* vals, int gx, int gy, uint32_t r_cap,
                                                        int32_t* __restrict__ n_touched, uint2* __restrict__ ranges,
                                                        int ntiles, uint32_t* __restrict__ zero_ptr, size_t zero_words,
                                                        uint32_t* __restrict__ count, uint32_t* __restrict__ overflow,
                                                        const uint32_t* __restrict__ depth_err, int offsets_global,
                                                        int scan_sh /* log2 of the scan block: offsets[] are local to it */,
                                                        int small_grid /* <= 2^16 tiles: dup_divmod */,
                                                        uint32_t* __restrict__ hist /* [4][256] or NULL */, int hist_passes,
                                                        int n_threads /* of this launch */, int slot_major,
                                                        unsigned long long* __restrict__ prepare /* GeometryState::prepare or NULL */) {
    const int i = blockIdx.x * 256 + threadIdx.x;          // (launched with 256 threads; blockDim would be a packet fetch)
    // the accumulator preprocess was asked to prepare goes to THIS render call's blend forward, and to no later one: the scratch
    // belongs to one backward, and a second render of the same geometry must not write into memory the caller may have freed
    if (i == 0 && prepare) {
        prepare[1] = prepare[0];
        prepare[0] = 0ull;
    }
    const int lane = threadIdx.x & 63;
    // Gaussian-major emission: every per-Gaussian input -- rectangle, depth key, the scanned offset of the Gaussian before and
    // its block's sum -- is requested HERE, before the housekeeping below, so that the wave waits for memory once.  (They
    // were three DEPENDENT round trips: the depth key, then the rectangle, then, only for a Gaussian that touches a tile,
    // the offset and the block sum -- most of the life of a wave that then emits ~170 pairs.)  Lanes past P load the
    // last Gaussian's and ignore them; a culled Gaussian's offset is read for nothing, which is cheaper than the trip.
    uint2 in_rect = make_uint2(0u, 0u);
    uint32_t in_gidx = 0, in_dkey = 0, in_off = 0, in_bsum = 0;
    if (!slot_major && P > 0) {                            // (grid-uniform)
        const int ci = i < P ? i : P - 1, cp = ci > 0 ? ci - 1 : 0;
        in_rect = rects[ci];                               // the rectangle preprocess computed (0 x 0: culled)
        in_off = offsets[cp];
        if (!offsets_global) in_bsum = block_sums[cp >> scan_sh];
        if (perm) {                                        // (global path: the key's address depends on perm -- one more trip)
            in_gidx = perm[ci];
            if (depth_key) in_dkey = depth_key[in_gidx];
        } else {
            in_gidx = (uint32_t)ci;
            if (depth_key) in_dkey = depth_key[ci];
        }
    }
    // a depth sort whose look-back timed out left perm / rect_sorted / offsets partly unwritten: emit nothing (the live
    // count is published as 0, so the tile sort, the ranges and the blend kernels have nothing to do either)
    const bool depth_bad = depth_err && radix_failed(depth_err) != 0u;
    uint32_t idx = 0, nt = 0, off = 0, kf = 0;
    int x0 = 0, y0 = 0, x1 = 0;
    // (an empty asm that "uses" the loaded values: the compiler otherwise sinks each load to its first use again)
    asm volatile("" ::"v"(in_rect.x), "v"(in_rect.y), "v"(in_gidx), "v"(in_dkey), "v"(in_off), "v"(in_bsum));
    if (i < P && !slot_major) {                          // everything in depth (or index) order and coalesced: no gather
        dup_pair(in_gidx, depth_key != nullptr, in_dkey, lo, idx, kf);
        const uint2 r = in_rect;
        const int w = (int)(r.y & 0xFFFFu), h = (int)(r.y >> 16);
        nt = (uint32_t)(w * h);
        x0 = (int)(r.x & 0xFFFFu); y0 = (int)(r.x >> 16); x1 = x0 + w;
    }
    if (depth_bad) nt = 0;                               // (wave-uniform, grid-uniform)
    if (nt) off = i == 0 ? 0u : in_off + in_bsum;
    // ---- housekeeping, behind the wait for the inputs: the wait then covers loads only (the memory counter is in order:
    //      a wait placed behind these stores would also wait for their acknowledgements)
    // scratch of the tile sort that follows (was its own launch)
    grid_zero(zero_ptr, zero_words, (size_t)n_threads, 256);
    if (i == 0 && count) {                               // capacity mode: live instance count + overflow flag (was a launch)
        const uint32_t R = (P > 0 && !depth_bad) ? block_sums[scan_nblocks_dev(P, scan_sh)] : 0u;
        count[0] = min(R, r_cap);
        count[1] = R > r_cap ? 1u : 0u;
    }
    // status word of this forward (see MGS_STATUS_* in monogs_raster.h): capacity overflow | depth-sort look-back timeout;
    // blend_forward_kernel adds the tile sort's flag
    if (i == 0 && overflow)
        overflow[0] = (count ? count[1] : 0u) | (depth_bad ? (uint32_t)MGS_STATUS_DEPTH_SORT_TIMEOUT : 0u);
    // empty-tile default, in the form the tile sort's final pass takes its minima / maxima over (blend_forward_kernel turns
    // what is still {~0, 0} afterwards into {0, 0})
    if (i < ntiles) ranges[i] = make_uint2(0xFFFFFFFFu, 0u);
    if (i < P) n_touched[i] = 0;                         // (was a memset)
    // Load-balanced emission.  The 64 Gaussians of the wave own the consecutive output slots [S, E); the wave walks
    // that range 64 slots at a time (aligned, so every store is one coalesced 256-byte line) and each lane finds the
    // owner of its slot: owners mark their first slot in LDS, an inclusive max-scan spreads the mark to the right.
    // A thread walking its own rectangle instead wrote 64 interleaved streams per wave (73 us at C5 for 26 MB).
    __shared__ uint32_t s_own[4][WAVE];
    __shared__ uint4 s_ent[4][WAVE];                                        // dup_entry
    __shared__ uint32_t s_kf[4][WAVE];
    const bool small = small_grid != 0;
    // Digit counts of the emitted tile ids (every pass of the tile sort), collected in LDS while the keys are written and
    // added to the global table once per workgroup: the one-sweep sort then needs no histogram launch of its own.
    __shared__ uint32_t s_hist[2][256];                                     // tile ids have <= 16 bits: two digits
    if (hist) {
        s_hist[0][threadIdx.x] = 0u; s_hist[1][threadIdx.x] = 0u;
        __syncthreads();
    }
    const int wv = threadIdx.x >> 6;
    if (slot_major) {
        // ---- emission balanced by OUTPUT SLOTS.  Gaussian-major (below), a wave owns the slots of its 64 Gaussians: in depth
        // order the near ones come first and cover hundreds of tiles each, so the first waves of the launch walk tens of
        // thousands of slots while most walk a few dozen (102 k Gaussians at 1200x680: 81 us for 1.3 M instances, against
        // 19 us for 5.3 M at C5 where every splat is small).  Here every wave of the launch owns an equal share [s0, s1) of
        // the slots, finds the Gaussian that owns s0 by a 64-way search of the scanned offsets (3 dependent probes at
        // 100 k Gaussians) and walks the Gaussians from there, 64 at a time, with the same owner-marking as below.
        const uint32_t R_all = (P > 0 && !depth_bad) ? block_sums[scan_nblocks_dev(P, scan_sh)] : 0u;
        const uint32_t R_emit = min(R_all, r_cap);
        const uint32_t n_waves = (uint32_t)n_threads / WAVE;
        const uint32_t CH = (((R_emit + n_waves - 1u) / n_waves) + 63u) & ~63u;
        const uint32_t wave_id = (uint32_t)blockIdx.x * 4u + (uint32_t)wv;
        const uint64_t s0w = (uint64_t)wave_id * CH;                             // (64-bit: wave_id * CH may pass 2^32 for R near 2^32)
        const uint32_t s0 = s0w < (uint64_t)R_emit ? (uint32_t)s0w : R_emit, s1 = (uint64_t)s0 + CH < (uint64_t)R_emit ? s0 + CH : R_emit;
        auto incl = [&](uint32_t k) { return offsets[k] + (offsets_global ? 0u : block_sums[k >> scan_sh]); };
        uint32_t g = 0;
        if (s0 < s1) {      // smallest g with incl(g) > s0: it exists because incl(P - 1) = R_all > s0
            uint32_t lo = 0, hi = (uint32_t)P;
            while (hi - lo > 1u) {
                const uint32_t span = hi - lo, step = (span + 63u) / 64u;
                const uint32_t probe = lo + min(((uint32_t)lane + 1u) * step, span) - 1u;
                const unsigned long long above = __builtin_amdgcn_ballot_w64(incl(probe) > s0);      // monotone in the lane
                const int k = __builtin_ctzll(above);                                                // (the last probe is hi - 1: set)
                const uint32_t pk = lo + min(((uint32_t)k + 1u) * step, span) - 1u;
                const uint32_t pk1 = k == 0 ? lo : lo + min((uint32_t)k * step, span);               // one past probe k - 1
                lo = pk1; hi = pk + 1u;
            }
            g = lo;
        }
        uint32_t sl = s0;
        while (sl < s1 && g < (uint32_t)P) {                                   // wave-uniform
            const uint32_t gi = g + (uint32_t)lane;
            const bool valid = gi < (uint32_t)P;
            uint32_t inc = 0, ntg = 0, idg = 0, kfg = 0;
            int gx0 = 0, gy0 = 0, gw = 1;
            if (valid) {
                inc = incl(gi);
                const uint2 r = rects[gi];
                gw = (int)(r.y & 0xFFFFu);
                ntg = (uint32_t)(gw * (int)(r.y >> 16));
                gx0 = (int)(r.x & 0xFFFFu); gy0 = (int)(r.x >> 16);
                const uint32_t pg = perm ? perm[gi] : gi;
                dup_pair(pg, depth_key != nullptr, depth_key ? depth_key[pg] : 0u, lo, idg, kfg);
            }
            const uint32_t exc = inc - ntg;                                    // first slot of the Gaussian
            uint32_t Eg = valid ? inc : 0u;                                    // end of the group's slots = the largest inclusive sum
            MGS_WAVE_REDUCE(Eg, max);
            __builtin_amdgcn_wave_barrier();
            s_ent[wv][lane] = dup_entry(exc, gx0, gy0, gw, gx, idg); s_kf[wv][lane] = kfg;
            const uint32_t e = min(s1, Eg);
            const uint32_t cb0 = sl & ~63u;
            const unsigned long long before = __builtin_amdgcn_ballot_w64(ntg != 0u && exc < cb0);
            uint32_t carry = before ? 64u - (uint32_t)__builtin_clzll(before) : 0u;      // owner (lane + 1) of the slot before the chunk
            for (uint32_t cb = cb0; cb < e; cb += WAVE) {
                __builtin_amdgcn_wave_barrier();
                s_own[wv][lane] = 0u;
                __builtin_amdgcn_wave_barrier();
                if (ntg != 0u && exc >= cb && exc < cb + WAVE) s_own[wv][exc - cb] = (uint32_t)lane + 1u;
                __builtin_amdgcn_wave_barrier();
                uint32_t m = s_own[wv][lane];
#define MGS_DPP_MAX(ctrl, row_mask) m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, ctrl, row_mask, 0xf, false))
                MGS_DPP_MAX(0x111, 0xf); MGS_DPP_MAX(0x112, 0xf); MGS_DPP_MAX(0x114, 0xf); MGS_DPP_MAX(0x118, 0xf);
                MGS_DPP_MAX(0x142, 0xa); MGS_DPP_MAX(0x143, 0xc);
#undef MGS_DPP_MAX
                const uint32_t owner = max(m, carry);
                carry = (uint32_t)__builtin_amdgcn_readlane((int)owner, 63);
                const uint32_t o = cb + lane;
                if (owner != 0u && o >= sl && o < e) {                        // (e <= R_emit <= r_cap: never past the buffers)
                    const uint32_t L = owner - 1u;
                    uint32_t key;
                    dup_emit(s_ent[wv][L], s_kf[wv][L], o, gx, tshift, small, keys, vals, key);
                    if (hist) {
                        atomicAdd(&s_hist[0][(key >> tshift) & 0xFFu], 1u);
                        if (hist_passes > 1) {      // (few values: the lanes that share the first active lane's digit add once)
                            const uint32_t d1 = (key >> (tshift + 8)) & 0xFFu;
                            const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)d1);
                            const unsigned long long same = __builtin_amdgcn_ballot_w64(d1 == lead);
                            if (d1 != lead) atomicAdd(&s_hist[1][d1], 1u);
                            else if (lane == (int)__builtin_ctzll(same)) atomicAdd(&s_hist[1][lead], (uint32_t)__popcll(same));
                        }
                    }
                }
            }
            sl = max(sl, e);
            if (Eg <= sl) g += WAVE;                                           // the group is used up
        }
        if (hist) {
            __syncthreads();
            const uint32_t c0 = s_hist[0][threadIdx.x], c1 = s_hist[1][threadIdx.x];
            if (c0) atomicAdd(hist + threadIdx.x, c0);
            if (c1) atomicAdd(hist + 256 + threadIdx.x, c1);
        }
        return;
    }
    s_ent[wv][lane] = dup_entry(off, x0, y0, x1 - x0, gx, idx); s_kf[wv][lane] = kf;
    const unsigned long long live = __builtin_amdgcn_ballot_w64(nt != 0);
    if (live == 0ull && !hist) return;                                      // wave-uniform
    const int first = live ? __builtin_ctzll(live) : 0, lastl = live ? 63 - __builtin_clzll(live) : 0;
    const uint32_t S = live ? (uint32_t)__builtin_amdgcn_readlane((int)off, first) : 0u;
    const uint32_t E = live ? (uint32_t)__builtin_amdgcn_readlane((int)(off + nt), lastl) : 0u;
    uint32_t carry = 0;                                                     // owner (lane + 1) of the slot before the chunk
    for (uint32_t cb = S & ~63u; cb < E; cb += WAVE) {
        __builtin_amdgcn_wave_barrier();
        s_own[wv][lane] = 0u;
        __builtin_amdgcn_wave_barrier();
        if (nt != 0 && off >= cb && off < cb + WAVE) s_own[wv][off - cb] = (uint32_t)lane + 1u;
        __builtin_amdgcn_wave_barrier();
        uint32_t m = s_own[wv][lane];
#define MGS_DPP_MAX(ctrl, row_mask) m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, ctrl, row_mask, 0xf, false))
        MGS_DPP_MAX(0x111, 0xf); MGS_DPP_MAX(0x112, 0xf); MGS_DPP_MAX(0x114, 0xf); MGS_DPP_MAX(0x118, 0xf);
        MGS_DPP_MAX(0x142, 0xa); MGS_DPP_MAX(0x143, 0xc);
#undef MGS_DPP_MAX
        const uint32_t owner = max(m, carry);
        carry = (uint32_t)__builtin_amdgcn_readlane((int)owner, 63);
        const uint32_t o = cb + lane;
        if (owner != 0u && o < E && o < r_cap) {                            // capacity mode: never write past the buffers
            const uint32_t L = owner - 1u;
            uint32_t key;
            dup_emit(s_ent[wv][L], s_kf[wv][L], o, gx, tshift, small, keys, vals, key);
            if (hist) {
                atomicAdd(&s_hist[0][(key >> tshift) & 0xFFu], 1u);
                if (hist_passes > 1) {
                    // the high digit takes a handful of values: the lanes that share the first active lane's digit add once
                    const uint32_t d1 = (key >> (tshift + 8)) & 0xFFu;
                    const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)d1);
                    const unsigned long long same = __builtin_amdgcn_ballot_w64(d1 == lead);
                    if (d1 != lead) atomicAdd(&s_hist[1][d1], 1u);
                    else if (lane == (int)__builtin_ctzll(same)) atomicAdd(&s_hist[1][lead], (uint32_t)__popcll(same));
                }
            }
        }
    }
    if (hist) {
        __syncthreads();
        const uint32_t c0 = s_hist[0][threadIdx.x], c1 = s_hist[1][threadIdx.x];
        if (c0) atomicAdd(hist + threadIdx.x, c0);
        if (c1) atomicAdd(hist + 256 + threadIdx.x, c1);
    }
}

// ------------------------------------------------------------------------------------------------
// Banded emission (ForwardPlan::bands != 0): duplicate_kernel's pairs, written grouped by band of 256 tiles.  One workgroup per
// scan block of 256 Gaussians.  The block's instances are its local slots [0, n) in Gaussian-major order (point_offsets[] are
// the block-local inclusive sums); a chunk of EB_CHUNK slots is decoded (owner of a slot: binary search of the 256 sums in
// LDS, then duplicate_kernel's slot decode), ranked stably by band with returning LDS atomics (the radix sort's ranking:
// lanes in ascending order, a wave's instructions in program order, the waves joined by a prefix), laid out band by band in
// an LDS stage and streamed to  band base + column scan of the band at this block + pairs of earlier chunks + rank.
// All counts are exact (preprocess counted them, scan_blocks_kernel scanned them): no atomics on global memory, no waiting.
// Capacity mode with fewer slots than instances: duplicate_kernel keeps the first r_cap slots of the Gaussian-major order, and so
// does this kernel -- the scan blocks before block B (the last one whose exclusive sum is <= r_cap) whole, the first
// r_cap - sum(B) slots of block B, nothing behind it.  The bands then hold fewer pairs than preprocess counted: EVERY
// workgroup finds B, decodes block B's kept slots and counts them per band itself (nobody waits for anybody; the overflowing
// forward is flagged and slow, not wrong), so that live total of band b = column scan of b at B + its share of block B.
// Workgroup 0 leaves the live totals in band_live[] for the segmented pass (without overflow: the totals themselves).
// Scan blocks are dealt to the workgroups one contiguous range per XCD (block ids go round-robin over the 8 XCDs), so that
// the short runs neighbouring blocks write into one band meet in one L2 -- the tile sort's xcd_band, for the same reason.
// ------------------------------------------------------------------------------------------------
constexpr int EB_THREADS = 256, EB_ITEMS = 4, EB_CHUNK = EB_THREADS * EB_ITEMS;
struct EmitBandedArgs {
    int P;
    const uint2* rects;
    const uint32_t* depth_key;
    int tshift, lo;
    const uint32_t* offsets;           // block-local inclusive sums
    const uint32_t* block_sums;        // [nblk] exclusive, [nblk] = total
    const uint32_t* band_counts;       // [nbands][nblk] exclusive along the blocks
    const uint32_t* band_totals;       // [nbands]
    uint32_t* band_live;               // [TILE_SORT_MAX_BANDS] out: pairs per band actually emitted
    int nbands, nblk;
    uint32_t* keys;
    uint32_t* vals;
    int gx;
    uint32_t r_cap;
    int32_t* n_touched;
    uint2* ranges;
    int ntiles;
    uint32_t* zero_ptr;
    size_t zero_words;
    uint32_t* count;
    uint32_t* overflow;
    const uint32_t* depth_err;
    int n_threads;
    unsigned long long* prepare;
};
__global__ void __launch_bounds__(EB_THREADS) emit_banded_kernel(EmitBandedArgs a) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int i = blockIdx.x * EB_THREADS + t;
    if (i == 0 && a.prepare) {                             // (see duplicate_kernel)
        a.prepare[1] = a.prepare[0];
        a.prepare[0] = 0ull;
    }
    const uint32_t nq = (uint32_t)a.nblk >> 3, nr = (uint32_t)a.nblk & 7u, xcd = blockIdx.x & 7u, j = blockIdx.x >> 3;
    const bool has = j < nq + (xcd < nr ? 1u : 0u);        // (workgroups past the scan blocks: housekeeping only)
    const uint32_t blk = has ? xcd * nq + min(xcd, nr) + j : 0u;
    // ---- every input requested before the housekeeping stores (see duplicate_kernel)
    const int gi = (int)blk * EB_THREADS + t, ci = gi < a.P ? gi : a.P - 1;
    const uint2 in_rect = a.rects[ci];
    const uint32_t in_off = a.offsets[ci], in_dkey = a.depth_key[ci];
    uint32_t in_bt = 0, in_bc = 0;
    if (t < a.nbands) {
        in_bt = a.band_totals[t];
        in_bc = a.band_counts[(size_t)t * a.nblk + blk];
    }
    const uint32_t R_all = a.block_sums[a.nblk];
    const bool depth_bad = a.depth_err && radix_failed(a.depth_err) != 0u;
    asm volatile("" ::"v"(in_rect.x), "v"(in_rect.y), "v"(in_off), "v"(in_dkey), "v"(in_bt), "v"(in_bc), "v"(R_all));
    // ---- housekeeping: duplicate_kernel's, word for word
    grid_zero(a.zero_ptr, a.zero_words, (size_t)a.n_threads, EB_THREADS);
    if (i == 0 && a.count) {
        const uint32_t R = !depth_bad ? R_all : 0u;
        a.count[0] = min(R, a.r_cap);
        a.count[1] = R > a.r_cap ? 1u : 0u;
    }
    if (i == 0 && a.overflow)
        a.overflow[0] = (a.count ? a.count[1] : 0u) | (depth_bad ? (uint32_t)MGS_STATUS_DEPTH_SORT_TIMEOUT : 0u);
    if (i < a.ntiles) a.ranges[i] = make_uint2(0xFFFFFFFFu, 0u);
    if (i < a.P) a.n_touched[i] = 0;
    if (!has || depth_bad) return;                         // (workgroup-uniform)

    __shared__ uint32_t s_incl[EB_THREADS];
    __shared__ uint4 s_ent[EB_THREADS];                    // dup_entry
    __shared__ uint32_t s_kf[EB_THREADS];
    __shared__ uint32_t s_cnt[EB_THREADS / WAVE][TILE_SORT_MAX_BANDS], s_dbase[TILE_SORT_MAX_BANDS], s_g[TILE_SORT_MAX_BANDS];
    __shared__ uint32_t s_k[EB_CHUNK], s_v[EB_CHUNK];
    uint32_t lim_blk = 0xFFFFFFFFu, lim_k = 0u;            // overflow: block lim_blk keeps its first lim_k slots
    if (R_all > a.r_cap) {                                 // (grid-uniform; see the header)
        uint32_t lo = 0u, hi = (uint32_t)a.nblk;           // block_sums[lo] <= r_cap < block_sums[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.block_sums[mid] <= a.r_cap) lo = mid; else hi = mid;
        }
        lim_blk = lo; lim_k = a.r_cap - a.block_sums[lo];
        const int g2 = (int)lim_blk * EB_THREADS + t, c2 = g2 < a.P ? g2 : a.P - 1;
        const uint2 r2 = a.rects[c2];
        const uint32_t off2 = a.offsets[c2];
        const int w2 = g2 < a.P ? (int)(r2.y & 0xFFFFu) : 0, h2 = g2 < a.P ? (int)(r2.y >> 16) : 0;
        s_incl[t] = off2;
        s_ent[t] = dup_entry(off2 - (uint32_t)(w2 * h2), (int)(r2.x & 0xFFFFu), (int)(r2.x >> 16), w2, a.gx, 0u);
        if (t < TILE_SORT_MAX_BANDS) s_dbase[t] = 0u;
        __syncthreads();
        for (uint32_t o = (uint32_t)t; o < lim_k; o += EB_THREADS) {
            uint32_t g = 0;
#pragma unroll
            for (uint32_t step = EB_THREADS / 2; step; step >>= 1)
                if (s_incl[g + step - 1u] <= o) g += step;
            const uint4 e = s_ent[g];
            uint32_t yy, xx;
            dup_divmod(o - e.x, e.z, true, yy, xx);
            atomicAdd(&s_dbase[(e.y + yy * (uint32_t)a.gx + xx) >> TILE_BAND_BITS], 1u);
        }
        __syncthreads();
        if (t < a.nbands) in_bt = a.band_counts[(size_t)t * a.nblk + lim_blk] + s_dbase[t];
        __syncthreads();                                   // (the arrays are filled again below)
    }
    if (blockIdx.x == 0 && t < TILE_SORT_MAX_BANDS) a.band_live[t] = in_bt;
    {
        const int w = gi < a.P ? (int)(in_rect.y & 0xFFFFu) : 0, h = gi < a.P ? (int)(in_rect.y >> 16) : 0;
        uint32_t val, kf;
        dup_pair((uint32_t)ci, true, in_dkey, a.lo, val, kf);
        s_incl[t] = in_off;                                // (lanes past P hold the last Gaussian's sum: the block's total)
        s_ent[t] = dup_entry(in_off - (uint32_t)(w * h), (int)(in_rect.x & 0xFFFFu), (int)(in_rect.x >> 16), w, a.gx, val);
        s_kf[t] = kf;
    }
    // band base (the prefix over the <= 32 band totals, formed in one wave) + what earlier scan blocks put into the band
    uint32_t gpos = 0;
    if (wv == 0) gpos = wave_incl_scan_dpp(in_bt) - in_bt + in_bc;
    __syncthreads();
    const uint32_t n_blk = blk < lim_blk ? s_incl[EB_THREADS - 1] : (blk == lim_blk ? lim_k : 0u);
    const int bshift = a.tshift + TILE_BAND_BITS;
    for (uint32_t c0 = 0; c0 < n_blk; c0 += EB_CHUNK) {    // (workgroup-uniform)
        if (t < (EB_THREADS / WAVE) * TILE_SORT_MAX_BANDS) s_cnt[t >> 5][t & 31] = 0u;
        __syncthreads();
        uint32_t key[EB_ITEMS], val[EB_ITEMS], rank[EB_ITEMS];
#pragma unroll
        for (int k = 0; k < EB_ITEMS; ++k) {
            const uint32_t o = c0 + (uint32_t)(wv * (EB_ITEMS * WAVE) + k * WAVE + lane);
            uint32_t g = 0;                                // the smallest g with s_incl[g] > o: the Gaussian that owns slot o
#pragma unroll
            for (uint32_t step = EB_THREADS / 2; step; step >>= 1)
                if (s_incl[g + step - 1u] <= o) g += step;
            const uint4 e = s_ent[g];
            uint32_t yy, xx;
            dup_divmod(o - e.x, e.z, true, yy, xx);
            key[k] = ((e.y + yy * (uint32_t)a.gx + xx) << a.tshift) | s_kf[g];
            val[k] = e.w;
            rank[k] = 0u;
            if (o < n_blk) rank[k] = __hip_atomic_fetch_add(&s_cnt[wv][key[k] >> bshift], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        if (wv == 0) {                                     // band `lane`: exclusive prefixes over the waves, then over the bands
            uint32_t tot = 0;
            if (lane < TILE_SORT_MAX_BANDS) {
#pragma unroll
                for (int w = 0; w < EB_THREADS / WAVE; ++w) {
                    const uint32_t c = s_cnt[w][lane];
                    s_cnt[w][lane] = tot;
                    tot += c;
                }
            }
            const uint32_t db = wave_incl_scan_dpp(tot) - tot;
            if (lane < TILE_SORT_MAX_BANDS) {
                s_dbase[lane] = db;
                s_g[lane] = gpos - db;                     // global position of stage slot 0 for the band, modulo 2^32
                gpos += tot;                               // ranks carry over to the next chunk
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < EB_ITEMS; ++k) {
            const uint32_t o = c0 + (uint32_t)(wv * (EB_ITEMS * WAVE) + k * WAVE + lane);
            if (o < n_blk) {
                const uint32_t b = key[k] >> bshift, slot = s_dbase[b] + s_cnt[wv][b] + rank[k];
                s_k[slot] = key[k];
                s_v[slot] = val[k];
            }
        }
        __syncthreads();
        const uint32_t chunk_n = min((uint32_t)EB_CHUNK, n_blk - c0);
#pragma unroll
        for (int k = 0; k < EB_ITEMS; ++k) {
            const uint32_t p = (uint32_t)(k * EB_THREADS + t);
            if (p < chunk_n) {
                const uint32_t kk = s_k[p], pos = s_g[kk >> bshift] + p;
                if (pos < a.r_cap) {                       // capacity mode: never write past the buffers
                    a.keys[pos] = kk;
                    a.vals[pos] = s_v[p];
                }
            }
        }
        // (the two barriers at the head of the next chunk stand between these reads and the next writes of s_g / the stage)
    }
}

static int launch_emit_banded(const ForwardPlan& plan, const GeometryState& g, const BinningState& b, const ImageState& img,
                              int32_t* n_touched, uint32_t* zero_ptr, size_t zero_words, uint32_t* count, uint32_t* overflow,
                              hipStream_t s) {
    EmitBandedArgs a;
    a.P = plan.P; a.rects = g.rect; a.depth_key = g.depth_key; a.tshift = plan.key_shift; a.lo = plan.depth_lo_bits;
    a.offsets = g.point_offsets; a.block_sums = g.scan_blocks; a.band_counts = g.band_counts; a.band_totals = g.band_totals;
    a.band_live = g.band_live; a.nbands = plan.bands; a.nblk = plan.scan_blocks;
    // the pairs go to the ping-pong side: the ONE pass that follows ends where two passes end
    a.keys = b.keys_b; a.vals = b.vals_b; a.gx = plan.tiles_x;
    a.r_cap = plan.r_cap < plan.R ? plan.r_cap : (uint32_t)plan.R;     // (never past the buffers, whatever the counts say)
    a.n_touched = n_touched; a.ranges = img.ranges; a.ntiles = plan.ntiles;
    a.zero_ptr = zero_ptr; a.zero_words = zero_words; a.count = count; a.overflow = overflow;
    a.depth_err = radix_depth_error_flag(g.sort_temp, (uint64_t)plan.P);
    const int tile_blocks = (a.ntiles + EB_THREADS - 1) / EB_THREADS;
    const int blocks = a.nblk > tile_blocks ? a.nblk : tile_blocks;
    a.n_threads = blocks * EB_THREADS;
    a.prepare = g.prepare;
    hipLaunchKernelGGL(emit_banded_kernel, dim3(blocks), dim3(EB_THREADS), 0, s, a);
    MGS_HIP(hipGetLastError());
    return 0;
}

// (also zeroes n_touched, the tile ranges and the scratch of the tile sort; in capacity mode it publishes the clamped live
//  count and the overflow flag; with R == 0 it emits nothing)
int launch_duplicate(const ForwardPlan& plan, const GeometryState& g, const BinningState& b, const ImageState& img,
                     int32_t* n_touched, uint32_t* count, uint32_t* overflow, hipStream_t s) {
    const int P = plan.P;
    const uint32_t* depth_err = P > 0 ? radix_depth_error_flag(g.sort_temp, (uint64_t)P) : nullptr;
    if (plan.dup_threads == 0) return 0;
    uint32_t* zero_ptr = nullptr;
    size_t zero_words = 0;
    g_dbg_last_tile_sort_bands = plan.bands;
    if (plan.R > 0) {
        if (plan.bands) radix_banded_zero_region(b.sort_temp, plan.R, plan.bands, &zero_ptr, &zero_words);
        else radix_zero_region(b.sort_temp, plan.R, plan.tile_bits, &zero_ptr, &zero_words);
    }
    if (plan.bands) return launch_emit_banded(plan, g, b, img, n_touched, zero_ptr, zero_words, count, overflow, s);
    // per-tile path: emission in Gaussian-index order with the depth bits packed into the pairs
    const bool per_tile = plan.per_tile;
    hipLaunchKernelGGL(duplicate_kernel, dim3(plan.dup_threads / 256), dim3(256), 0, s, P, per_tile ? g.rect : g.rect_sorted,
                       per_tile ? nullptr : g.perm, per_tile ? g.depth_key : nullptr, plan.key_shift, plan.depth_lo_bits,
                       g.point_offsets, g.scan_blocks, b.keys_a, b.vals_a, plan.tiles_x, plan.tiles_y, plan.r_cap, n_touched,
                       img.ranges, plan.ntiles, zero_ptr, zero_words, count, overflow, depth_err, plan.scan_small ? 1 : 0,
                       plan.scan_shift, plan.small_grid ? 1 : 0, plan.count_digits ? g.tile_hist : nullptr,
                       (plan.tile_bits + 7) / 8, plan.dup_threads, plan.slot_major ? 1 : 0, P > 0 ? g.prepare : nullptr);
    MGS_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// the two stable sorts (radix_sort.hip)
// ------------------------------------------------------------------------------------------------
size_t sort_temp_bytes(uint64_t n, int bits) { return radix_temp_bytes(n, bits); }

int launch_depth_sort(const ForwardPlan& plan, const GeometryState& g, hipStream_t s) {
    // the scratch was cleared by preprocess_forward_kernel; the final pass also lays the tile rectangles out in depth
    // order for the scan and duplicate (rect_packed: they travelled with the pairs, else it gathers them)
    return radix_sort_depth(g.depth_key, g.depth_alt, g.iota, g.iota_alt, g.rect, plan.rect_packed, g.perm, g.rect_sorted,
                            (uint64_t)plan.P, g.sort_temp, s, true, plan.exclusive);
}

int launch_sort(const ForwardPlan& plan, const GeometryState& g, const BinningState& b, const ImageState& img,
                const uint32_t* n_dev, hipStream_t s) {
    if (plan.R == 0) return 0;
    // banded: emit_banded_kernel left the pairs grouped by band on the ping-pong side; one segmented pass on the low 8 tile bits
    if (plan.bands)
        return radix_sort_banded(b.keys_b, b.vals_b, b.keys_a, b.vals_a, plan.R, plan.key_shift, b.sort_temp, s, n_dev, g.band_live,
                                 plan.bands, img.ranges);
    // the scratch was cleared by duplicate_kernel, which also counted the digits of the keys it emitted (plan.count_digits;
    // never a NULL histogram).  Per-tile depth order: the tile id is the top tile_bits of the key, the depth bits ride along.
    RadixSortOptions o;
    o.n_dev = n_dev; o.temp_zeroed = true; o.exclusive = plan.exclusive;
    o.ext_hist = (plan.count_digits && g.tile_hist != nullptr) ? g.tile_hist : nullptr;
    o.ranges = img.ranges; o.key_shift = plan.key_shift;      // (the final pass writes the per-tile ranges)
    return radix_sort_pairs(b.keys_a, b.vals_a, b.keys_b, b.vals_b, plan.R, plan.tile_bits, b.sort_temp, s, o);
}

// ------------------------------------------------------------------------------------------------
// Per-tile depth order (ForwardPlan::sort_tiles: large maps): tile_sort.h.  By default blend_forward_kernel<true> sorts its
// own tile's list before it walks it (option "tile_sort_fused"); this kernel is the same sort as a launch of its own,
// one 256-thread workgroup per tile.
// ------------------------------------------------------------------------------------------------
TileSortArgs tile_sort_args(const ForwardPlan& plan, const GeometryState& g, const BinningState& b, const uint32_t* n_dev) {
    TileSortArgs ts;
    ts.keys = b.keys_sorted; ts.vals = b.vals_sorted;
    ts.keys_alt = b.keys_sorted == b.keys_a ? b.keys_b : b.keys_a;
    ts.vals_alt = b.vals_sorted == b.vals_a ? b.vals_b : b.vals_a;
    ts.depth_key = g.depth_key; ts.n_dev = n_dev;
    ts.n_cap = (uint32_t)plan.R; ts.tb = plan.tile_bits;
    return ts;
}

__global__ void __launch_bounds__(TDS_THREADS) tile_depth_sort_kernel(TileSortArgs ts, const uint2* __restrict__ ranges,
                                                                       int ntiles, const uint32_t* __restrict__ sort_err) {
    __shared__ uint32_t s_k[TDS_CAP], s_v[TDS_CAP];
    __shared__ uint32_t s_cnt[TDS_WAVES][TDS_RADIX];
    __shared__ uint32_t s_wsum[TDS_WAVES], s_red[2 * TDS_WAVES];
    const int tile = blockIdx.x;
    if (tile >= ntiles) return;
    // a timed-out tile sort left the ranges invalid: blend_forward_kernel empties every tile, nothing to order here
    tile_depth_sort(ts, ranges[tile], sort_err && radix_failed(sort_err) != 0u, TdsLds{s_k, s_v, s_cnt, s_wsum, s_red});
}

int launch_tile_depth_sort(const ForwardPlan& plan, const TileSortArgs& ts, const ImageState& img, const uint32_t* sort_err,
                           hipStream_t s) {
    hipLaunchKernelGGL(tile_depth_sort_kernel, dim3(plan.ntiles), dim3(TDS_THREADS), 0, s, ts, img.ranges, plan.ntiles, sort_err);
    MGS_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// tile ranges: written by the tile sort's final pass (radix_sort.hip, RsPassArgs::ranges) since round 4 -- the kernel that
// compared neighbouring sorted keys (one launch, 4 R bytes of reads) is gone; blend_forward_kernel checks the sort's error
// words and normalises the empty tiles.
// ------------------------------------------------------------------------------------------------

}  // namespace mgs
