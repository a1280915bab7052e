// The forward's route, stated once ("The forward plan").  One forward takes one of several routes through the same
// kernels; every decision that picks the route is a field here, made by ONE builder (binning.hip) and read by every launcher.
// No launcher derives a field for itself: a new route is one field and one rule in the builder.
//
//   const ForwardPlan pre = forward_plan(P, W, H, cam.flags);     // mgs_forward_preprocess: the first half
//   const ForwardPlan plan = pre.render(R, capacity_mode);        // forward_render_impl: both halves
//
// The builder is a pure function of its arguments and of the mgs_debug_set_option values at the time of the call;
// mgs_debug_forward_plan shows its answer (one word per field, MGS_PLAN_* in include/monogs_raster.h).
#pragma once

#include <stdint.h>

namespace mgs {

struct ForwardPlan {
    // ---- inputs
    int P, W, H, flags;
    bool capacity_mode;        // render half: R is the capacity of the binning buffers, the live count stays on the device
    // ---- geometry
    int tiles_x, tiles_y, ntiles;
    int tile_bits;             // bits of the tile id that can be set
    bool small_grid;           // ntiles <= 65536: duplicate_kernel's `small` (dup_divmod)
    // ---- preprocess half: known from (P, W, H, flags) and the options
    bool per_tile;             // depth order per tile (tile_sort.h), no global depth sort
    int scan_items;            // Gaussians per scan block: SCAN_ITEMS_PRE when preprocess scans, else SCAN_ITEMS
    int scan_shift;            // log2(scan_items): how the granularity travels to the kernels
    int scan_blocks;           // ceil(P / scan_items); the grand total lies at scan_blocks[this]
    bool scan_small;           // the single-launch scan (SCAN_ITEMS granularity only: it writes GLOBAL sums)
    int bands_counted;         // bands of 256 tiles that preprocess counts and the scan launch scans (0: none)
    bool rect_packed;          // the depth sort carries the packed rectangles as a payload (else its last pass gathers them)
    bool exclusive;            // MGS_FLAG_EXCLUSIVE_DEVICE
    // ---- render half: known once the instance count (or the capacity) R is -- render()
    uint64_t R;                // 0 when P == 0
    uint32_t r_cap;            // the emission's bound: the capacity; on the exact path 0xFFFFFFFF, or 0 when R == 0
    bool slot_major;           // duplicate_kernel balanced by output slots, not by Gaussians
    int bands;                 // the banded emission + ONE segmented tile-sort pass (0: the plain emission and two passes,
                               // whatever preprocess counted)
    bool count_digits;         // duplicate_kernel counts the tile sort's digits: the sort launches no histogram kernel
    int key_shift;             // per-tile path: the tile id is the top tile_bits of the key (32 - tile_bits); else 0
    int depth_lo_bits;         // per-tile path: depth bits that ride in the value (tile_depth_lo_bits); else 0
    bool sort_tiles;           // per-tile path with instances: every tile's list is sorted by depth
    bool tile_sort_fused;      // ... by the blend forward's workgroup of the tile (else a launch of its own)
    int dup_threads;           // threads of the duplicate_kernel launch

    ForwardPlan render(uint64_t R, bool capacity_mode) const;
};
ForwardPlan forward_plan(int P, int W, int H, int flags);

}  // namespace mgs
