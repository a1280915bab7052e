/* monogs_raster.h -- C ABI of libmonogs_raster.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the native operators MonoGS calls (the third, fused_ssim -- imported at
 * /root/reference/gaussian_splatting/utils/loss_utils.py:19 -- is described at mgs_ssim_forward below):
 *
 *   diff_gaussian_rasterization   imported at /root/reference/gaussian_splatting/gaussian_renderer/__init__.py:13-16,
 *                                 settings built at :70-84, called at :130-156
 *   simple_knn._C.distCUDA2       imported at /root/reference/gaussian_splatting/scene/gaussian_model.py:18,
 *                                 called at :294-302
 *
 * The reference binds these through pybind11 + torch::Tensor (there is no C plugin ABI upstream; the
 * sources are un-vendored submodules, /root/reference/.gitmodules:1-6).  This header is the C-level
 * contract of the same entry points: plain device pointers, sizes and a HIP stream; no torch types.
 * The entry points correspond 1:1 to the upstream extension functions listed in SURVEY.md section 8b:
 *
 *   rasterize_gaussians            -> mgs_forward_preprocess + mgs_forward_render
 *   rasterize_gaussians_backward   -> mgs_backward
 *   mark_visible                   -> mgs_mark_visible
 *   distCUDA2                      -> mgs_dist2_knn
 *
 * Conventions
 *   - every pointer is DEVICE memory on the current HIP device unless marked [host];
 *   - float tensors are contiguous float32; matrices are the 4x4 tensors MonoGS passes, i.e. the
 *     TRANSPOSE of the maths matrix (flat element 4*j+i is maths element (i,j));
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *   - every function returns 0 on success and a non-zero code on failure; mgs_last_error() gives the
 *     message of the calling thread's last failure;
 *   - the library keeps no state between calls: scratch lives in caller-owned buffers whose sizes come
 *     from the mgs_*_bytes functions, so several forwards may precede one backward
 *     (/root/reference/utils/slam_mapper.py:273-394) and several processes may share a GPU.
 */
#ifndef MONOGS_RASTER_H
#define MONOGS_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGS_ABI_VERSION 31
#define MGS_TILE 16 /* tile edge in pixels; ranges are per 16x16 tile */

/* GaussianRasterizationSettings, minus `prefiltered` / `debug` which are call flags
 * (/root/reference/gaussian_splatting/gaussian_renderer/__init__.py:70-84). */
typedef struct mgs_camera {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    float scale_modifier;
    int32_t sh_degree;           /* active SH degree (0..3); ignored with colors_precomp */
    int32_t sh_coeffs;           /* M: coefficient triplets per Gaussian in `shs` (0 with colors_precomp) */
    int32_t scale_dim;           /* floats per Gaussian in `scales` / `dL_dscales`: 0 or 3 = (sx, sy, sz); 1 = isotropic --
                                    the expansion render() does with scales.repeat(1, 3)
                                    (/root/reference/gaussian_splatting/gaussian_renderer/__init__.py:101-104) and the
                                    sum of its backward happen inside the kernels */
    int32_t flags;               /* MGS_FLAG_* bits, 0 = none */
    const float* bg;             /* [3]  */
    const float* viewmatrix;     /* [16] transposed world->camera */
    const float* projmatrix;     /* [16] transposed P @ T_cw */
    const float* projmatrix_raw; /* [16] transposed P */
    const float* campos;         /* [3]  */
} mgs_camera;

/* mgs_camera.flags.
 * MGS_FLAG_EXCLUSIVE_DEVICE: the caller guarantees that NO other grid runs beside this call's kernels -- one process on the
 * device, one stream (a pose-tracking loop, a captured single-stream iteration).  The small radix sorts (<= 256 tiles) and
 * the single-launch scan then take their tile / block ids from the block index, which saves a returning atomic (~2 us) per
 * launch.  Without the flag -- the default, and what MonoGS's topology needs: tracker, mapper and viewer processes share one GPU
 * (/root/reference/slam.py:102-179), and a mapping window renders its keyframes on a stream each -- every such launch hands out
 * its ids by an atomic ticket, so a workgroup only ever waits for workgroups that have already started: forward progress does not
 * depend on where, or in which order, the hardware places workgroups of competing grids. */
#define MGS_FLAG_EXCLUSIVE_DEVICE 1
/* MGS_FLAG_INTRINSICS_GRAD (ABI v28): mgs_backward also sums dL/d(fx, fy, cx, cy), the gradient with respect to the pinhole
 * intrinsics in pixels, with projmatrix_raw depending on them as P00 = 2 fx / W, P11 = 2 fy / H, P02 = (2 cx - W) / W,
 * P12 = (2 cy - H) / H and tanfovx = W / (2 fx), tanfovy = H / (2 fy).  Culling, radius, tile rectangle and the 1.3 tanfov
 * clamp test are constants, as they are for the pose gradient.  dL_dtau is then TEN floats (rho, theta, dfx, dfy, dcx, dcy)
 * and must not be NULL.  The four sums take the path of the pose gradient -- floats 6..9 of the same 16-float lines, the same
 * float atomics across workgroups, so the same reproducibility: deterministic up to the order of those adds.  The forward
 * entry points ignore the bit. */
#define MGS_FLAG_INTRINSICS_GRAD 2

/* Per-stage device time in milliseconds, measured with HIP events on `stream`.
 * Passing a non-NULL mgs_timing makes the call synchronise `stream` before returning. */
typedef struct mgs_timing {
    float preprocess_ms;
    float depth_sort_ms;
    float scan_ms;
    float duplicate_ms;
    float sort_ms;        /* the tile sort; on the per-tile path (mgs_binning_path) also the per-tile depth sort when it runs as a
                             launch of its own (option "tile_sort_fused" = 0) -- by default it runs inside the blend forward */
    float ranges_ms;      /* always 0 since ABI v8: the tile sort's final pass writes the ranges (kept for layout compatibility) */
    float blend_fwd_ms;   /* per-tile path, by default: includes the per-tile depth sort */
    float blend_bwd_ms;
    float geom_bwd_ms;
} mgs_timing;

int mgs_abi_version(void);
const char* mgs_last_error(void);

/* Largest map one call takes.  The blend backward addresses a Gaussian's 64-byte gradient line with a 32-bit byte offset
 * (index x 64 + slot), which wraps at 2^26 Gaussians; the entry points that take P return 1 ("P exceeds ...") beyond it
 * instead of wrapping.  (A 288 GB device could hold such a map; MonoGS maps are 10^4 .. 10^6.) */
#define MGS_MAX_GAUSSIANS ((1 << 26) - 1)

/* Scratch sizes (bytes).  geometry: per-Gaussian state carried from forward to backward;
 * image: per-pixel and per-tile state; binning: keys / values / sort temp for R = num_rendered.
 * LIFETIME (caller-owned, the library keeps nothing): geometry, image, binning and the backward scratch must stay
 * allocated and unmodified from the forward until the LAST backward through it has run; radii / n_touched / the three
 * images are plain outputs and need not outlive anything.  The Python binding (monogs_amd/rasterizer.py) carries the
 * scratch in the autograd context -- about 250 B per Gaussian + 8 B per pixel + 16 B per instance, alive exactly as long as
 * the graph of that forward -- and hands out radii / n_touched as views of their own 8 P-byte tensor and the images as views
 * of one 20 HW-byte tensor, so keeping an OUTPUT (render_pkg["radii"], a keyframe's n_touched) never pins the scratch. */
size_t mgs_geometry_bytes(int32_t P);
size_t mgs_image_bytes(int32_t width, int32_t height);
size_t mgs_binning_bytes(uint64_t num_rendered, int32_t width, int32_t height);
size_t mgs_backward_bytes(int32_t P);
/* The floats inside a backward scratch that a PREPARED backward (below) accumulates dL/dtau into: a 64-byte line of which the
 * first six are used -- the first ten with MGS_FLAG_INTRINSICS_GRAD.  The preparing forward clears the whole line. */
float* mgs_backward_tau(void* backward_scratch, int32_t P);
/* TEST USE ONLY, pure: byte offset (from the 256-byte-aligned base the carving uses) and length of a named
 * sub-buffer; non-zero with mgs_last_error() set for an unknown name.  This export is the statement of the scratch layout:
 * tests and tools ask here and compute no offset of their own.
 * Names: a caller may rely on "<scratch>.<member>" with <scratch> one of geometry (sized by P), image (W, H), binning
 * (R, W, H), backward (P) and <member> as csrc/common.h spells it (geometry.rec, image.ranges, binning.fwd_masks,
 * backward.grad_acc, ...), plus "binning.point_list": the Gaussian index per instance in blend order, i.e. whichever of
 * vals_a / vals_b the tile sort's pass count leaves its result in.
 * Alignment: the base is the scratch pointer rounded up to 256 bytes; every sub-buffer of the geometry, image and binning
 * scratch starts at a multiple of 256 from it, every one of the backward scratch at a multiple of 64. */
int mgs_debug_scratch_field(const char* field, int32_t P, uint64_t R, int32_t W, int32_t H,
                            uint64_t* offset, uint64_t* bytes);

/* Forward, stage 1: per-Gaussian projection (cull, covariance, radius, tile rectangle, colour), the depth
 * order of the Gaussians and the prefix sum of tiles touched in that order.  Writes radii[P] and the geometry scratch, then copies the total number
 * of (Gaussian, tile) instances to *num_rendered [host] -- this synchronises `stream`, exactly as the
 * upstream forward does, because the caller must size the binning scratch from it.
 * Exactly one of (shs, colors_precomp) and exactly one of ((scales, rotations), cov3D_precomp) is non-NULL.
 * `prepare_backward`: NULL, or the scratch (mgs_backward_bytes(P)) of the ONE backward that will follow this forward.
 * The forward then also clears what that backward accumulates into: the per-Gaussian kernel the pose-gradient slots and the
 * six floats at mgs_backward_tau(scratch, P), and the blend forward of the render call that follows (mgs_forward_render,
 * mgs_forward_render_capacity) the P 64-byte gradient lines -- the scratch is prepared once BOTH calls have run, and
 * mgs_backward may then be called with scratch_prepared = 1: no clearing launch per backward.  The address travels in the
 * geometry scratch and is good for ONE render call: a later render of the same geometry scratch clears nothing. */
int mgs_forward_preprocess(const mgs_camera* cam, int32_t P,
                           const float* means3D,        /* [P,3] */
                           const float* shs,            /* [P,M,3] or NULL */
                           const float* colors_precomp, /* [P,3] or NULL */
                           const float* opacities,      /* [P] */
                           const float* scales,         /* [P,3] or NULL */
                           const float* rotations,      /* [P,4] or NULL */
                           const float* cov3D_precomp,  /* [P,6] or NULL */
                           void* geometry, int32_t* radii /* [P] */,
                           void* prepare_backward /* backward scratch to clear, or NULL */,
                           uint64_t* num_rendered /* [host]; NULL = capacity mode, no sync */,
                           const uint32_t* prev_status /* device, optional: status word of an EARLIER forward on this stream */,
                           uint32_t* prev_status_out /* [host], optional: receives *prev_status at this call's own
                                                        synchronisation (num_rendered != NULL): a sort timeout of the exact
                                                        path cannot pass unseen, and costs no synchronisation of its own */,
                           mgs_timing* timing /* [host] or NULL */, void* stream);

/* Forward, stage 2: duplicate (in depth order, or in index order -- mgs_binning_path), stable grouping by tile, per-tile ranges, front-to-back blend.
 * Outputs: color[3,H,W], depth[1,H,W] (sum z.alpha.T), opacity[1,H,W] (1 - T), n_touched[P]
 * (zeroed here, then incremented per pixel where the Gaussian is blended with T.(1-alpha) > 0.5). */
int mgs_forward_render(const mgs_camera* cam, int32_t P, uint64_t num_rendered,
                       void* geometry, void* binning, void* image,
                       float* out_color, float* out_depth, float* out_opacity, int32_t* n_touched,
                       uint32_t* status /* device, optional: MGS_STATUS_* bits of this forward */,
                       mgs_timing* timing, void* stream);

/* Status word of a forward (device uint32, written by the forward's own kernels; 0 = clean).  The hand-written radix
 * sort bounds every inter-workgroup wait (small sorts only: a tile waits for the digit counts of earlier tiles); a wait
 * that runs out raises a flag instead of hanging, and the sorted order (hence the blend order) is then invalid.  mgs_forward_preprocess reports a depth-sort timeout itself when it
 * synchronises (num_rendered != NULL); everything else arrives here and is read by the caller at a sync point of its
 * choice (monogs_amd.rasterizer.check_overflow). */
#define MGS_STATUS_CAPACITY_OVERFLOW 1u   /* capacity mode: instances were dropped */
#define MGS_STATUS_DEPTH_SORT_TIMEOUT 2u  /* a bounded wait of the depth sort ran out */
#define MGS_STATUS_TILE_SORT_TIMEOUT 4u   /* a bounded wait of the tile sort ran out */

/* ---- mgs_debug_*: TEST AND MEASUREMENT USE ONLY -------------------------------------------------------------------------
 * "The library keeps no state between calls" (above) holds for every entry point a caller of the rasteriser needs.  The three
 * setters below are the exception, on purpose: each writes a PROCESS-GLOBAL variable that later calls read unsynchronised.
 * They are NOT THREAD-SAFE (set them while no other thread is inside the library), they affect every later call of the process
 * whatever its device or stream, and nothing on MonoGS's path calls them: the test suite and the tools under tools/ do, to force
 * an algorithm path or to time a kernel.  Defaults are restored by the values given with each. */
/* TEST USE ONLY, process-global, not thread-safe: the bound of those waits, in polls (all later sorts); 0xFFFFFFFF restores the default. */
int mgs_debug_set_radix_spin_limit(uint32_t limit);
/* TEST USE ONLY, process-global, not thread-safe: knobs that force an algorithm path whatever the problem size (one table in csrc/api.hip; any negative value, -1 by convention, restores the default of EVERY knob):
 * "radix_scanned" (0 = one kernel per pass with a gather of the earlier tiles' counts, 1 = counted tiles: two kernels per
 * pass, no waiting between workgroups -- honoured from 64 k pairs), "radix_ballot_rank" (1 = rank with wave ballots instead of
 * returning LDS atomics: the reference the sort tests compare with), "scan_small" (0 = the two-launch scan at every size),
 * "pre_scan" (per-tile path, mgs_binning_path() == 1: -1 / 1 = default, the per-Gaussian forward kernel scans the tiles touched
 * by its own workgroup's 256 Gaussians and one launch scans the block sums -- "scan_small" then has no effect there; 0 = the
 * scan as launches of its own over the rectangles, as on the global path.  Set it between whole forwards, not between
 * mgs_forward_preprocess and the render call that consumes its geometry scratch; the same tables either way),
 * "dup_slot_major" (0 / 1 = the duplicate kernel's emission balanced by Gaussians / by output slots at every size),
 * "tile_sort_fused" (per-tile path: 1 = default, each blend forward workgroup sorts its own tile's list first; 0 = the
 * per-tile depth sort as a launch of its own between the tile sort and the blend forward; the same lists either way),
 * "knn_grid_min" (Morton-box kNN from this many points), "blend_bwd_transposed" (2 = default, 1 = round 3's transposed blend
 * backward fed by per-survivor scalar loads, 0 = the per-survivor wave reduction; a value set by hand names that one kernel:
 * once 2 has been SET, it is the unsplit walk FOR THE REST OF THE PROCESS -- also for callers that only meant "the default" --
 * until "blend_bwd_split" says otherwise or "blend_bwd_transposed" is set to -1, which alone restores the default),
 * "blend_bwd_split" (with blend_bwd_transposed = 2 and the forward's images given to mgs_backward: 1 = every quadrant's list is
 * walked by two waves, its front part front to back and the rest back to front, all back parts launched first; 2 = the same
 * with the two parts of a tile in adjacent workgroups; 0 = one wave walks the whole list; -1 = the default: 1 from a mean
 * list of 128 instances per tile, if "blend_bwd_transposed" has not been set by hand; the count is mgs_backward's
 * num_rendered, i.e. in capacity mode the CAPACITY, so the line moves with the caller's headroom),
 * "blend_bwd_split_min" / "blend_bwd_split_frac" (the shortest list that is split, in 64-instance steps, default 4; the
 * front walk's share of a list in 256ths, default 32),
 * "radix_xcd_band" (0 = counted tiles in block-id order instead of one contiguous band of tiles per XCD),
 * "debug_sort_exclusive" (1 = mgs_debug_sort_pairs sorts as under MGS_FLAG_EXCLUSIVE_DEVICE).  Nothing on the launch path
 * consults the environment. */
int mgs_debug_set_option(const char* name, int64_t value);

/* Which depth order a forward of P Gaussians at W x H builds (pure; follows the "radix_scanned" option, process-global):
 * 0 = a global stable sort of the P depth keys, the instances emitted in that order and grouped by tile;
 * 1 = per tile: the instances emitted in Gaussian-index order with their depth bits packed into the tile sort's pairs,
 *     grouped by tile, and each tile's list sorted by (depth bits, index) in LDS -- taken where the depth sort would
 *     take the counted-tiles path (P > 512 k, or any P with "radix_scanned" = 1), the tile id has <= 16 bits and
 *     P <= 2^(37 - tile bits).  Both orders are identical; what the geometry scratch holds differs (monogs_amd/debug.py, forward_tables). */
int mgs_binning_path(int32_t P, int32_t W, int32_t H);

/* Test entry: the library's stable radix sort of n (key, value) pairs on key bits [0, bits) -- what the forward runs on
 * the depth keys and on the tile ids -- on caller-provided DEVICE buffers: keys / vals hold the input and receive the
 * sorted pairs, keys_alt / vals_alt (n words each) are the ping-pong partners, temp (mgs_debug_sort_temp_bytes(n, bits)
 * bytes) the scratch.  Returns non-zero with mgs_last_error() set if a look-back spin timed out. */
size_t mgs_debug_sort_temp_bytes(uint64_t n, int32_t bits);
int mgs_debug_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t* keys_alt, uint32_t* vals_alt, uint64_t n, int32_t bits,
                         void* temp, void* stream);

/* Forward, stage 2 without a host-side instance count ("capacity mode"): call mgs_forward_preprocess with
 * num_rendered = NULL (no read-back, no stream sync), size the binning scratch with
 * mgs_binning_bytes(capacity, W, H) for a caller-chosen capacity (e.g. 1.5x the previous frame's count), and the
 * kernels read the live count min(R, capacity) on the device.  If R > capacity the surplus instances are dropped
 * and MGS_STATUS_CAPACITY_OVERFLOW is set in *overflow (device uint32, optional; the forward's status word, which
 * also receives the sort-timeout bits): the caller must re-render with a larger capacity.  The
 * whole forward + backward then contains no host synchronisation and can be captured in a hipGraph.
 * Pass the same `capacity` as num_rendered to mgs_backward. */
int mgs_forward_render_capacity(const mgs_camera* cam, int32_t P, uint64_t capacity,
                                void* geometry, void* binning, void* image,
                                float* out_color, float* out_depth, float* out_opacity, int32_t* n_touched,
                                uint32_t* overflow, mgs_timing* timing, void* stream);
/* Both stages of a capacity-mode forward in ONE call (mgs_forward_preprocess with num_rendered = NULL, then
 * mgs_forward_render_capacity): what an eager caller pays per crossing of the FFI boundary matters at SLAM sizes. */
int mgs_forward_capacity(const mgs_camera* cam, int32_t P, const float* means3D, const float* shs,
                         const float* colors_precomp, const float* opacities, const float* scales, const float* rotations,
                         const float* cov3D_precomp, void* geometry, int32_t* radii, void* prepare_backward,
                         uint64_t capacity, void* binning, void* image, float* out_color, float* out_depth,
                         float* out_opacity, int32_t* n_touched, uint32_t* overflow, mgs_timing* timing, void* stream);

/* Backward.  Consumes dL/dcolor[3,H,W] and dL/ddepth[1,H,W] (dL/dopacity is ignored, as upstream) and
 * the scratch of the matching forward.  Any output pointer may be NULL (that gradient is then not
 * stored); dL_dtau is [6] = (rho, theta), already summed over Gaussians -- with MGS_FLAG_INTRINSICS_GRAD in cam->flags it is
 * [10] = (rho, theta, dfx, dfy, dcx, dcy) and must not be NULL (return 1 with a message before any launch).
 * scratch_prepared = 1: `backward_scratch` was handed to the matching mgs_forward_preprocess as prepare_backward and has
 * not been used by a backward since; dL_dtau must then be NULL or mgs_backward_tau(backward_scratch, P).
 * `out_color` [3,H,W] and `out_depth` [1,H,W] are the images the matching forward wrote, unchanged; with them the blend
 * backward may walk every pixel list from both ends at once (two waves per quadrant).  Either may be NULL: the lists are
 * then walked from the back only -- the same gradients to rounding, a longer kernel on large images. */
int mgs_backward(const mgs_camera* cam, int32_t P, uint64_t num_rendered,
                 const float* means3D, const float* shs, const float* colors_precomp,
                 const float* opacities, const float* scales, const float* rotations,
                 const float* cov3D_precomp, const int32_t* radii,
                 const void* geometry, const void* binning, const void* image,
                 const float* dL_dcolor, const float* dL_ddepth,
                 const float* out_color, const float* out_depth,
                 float* dL_dmeans2D,  /* [P,3] NDC-scaled x,y; z = 0 */
                 float* dL_dcolors,   /* [P,3] (colors_precomp) */
                 float* dL_dopacity,  /* [P]   */
                 float* dL_dmeans3D,  /* [P,3] */
                 float* dL_dcov3D,    /* [P,6] (cov3D_precomp) */
                 float* dL_dsh,       /* [P,M,3] (shs) */
                 float* dL_dscales,   /* [P,3] */
                 float* dL_drotations,/* [P,4] */
                 float* dL_dtau,      /* [6], or [10] with MGS_FLAG_INTRINSICS_GRAD */
                 void* backward_scratch, int32_t scratch_prepared, mgs_timing* timing, void* stream);

/* Diagnostic: MGS_VALU_CEILING_BLOCKS x 256 threads (8 waves per SIMD on all 256 compute units) run `iters` trips of 8
 * independent v_fma_f32 each and store one float per thread into out[MGS_VALU_CEILING_BLOCKS * 256].  Timed by the caller,
 * 8 * iters * MGS_VALU_CEILING_BLOCKS * 4 wave-instructions / time is the plain-FMA issue rate this chip sustains (the
 * ceiling bench.py quotes next to the 1228.8 G wave-inst/s of the data sheet). */
#define MGS_VALU_CEILING_BLOCKS 2048
int mgs_debug_valu_ceiling(float* out, int32_t iters, void* stream);

/* TEST / MEASUREMENT USE ONLY, process-global, not thread-safe.
 * Measurement hook: until switched off again, every forward records fwd_start right before and fwd_end right after its
 * blend-forward launch, every mgs_backward bwd_start / bwd_end around its blend-backward launch, on the call's stream
 * (hipEvent_t handles owned by the caller, created with timing enabled; each pair both set or both NULL; four NULLs switch
 * the hook off).  No synchronisation, nothing else changes: bench.py times the two blend kernels INSIDE its timed region
 * with it (an mgs_timing struct synchronises per call, and a device that idles between kernels clocks the issue-bound
 * blend kernels ~8 % slower than back-to-back steps do).  Process-wide, not thread-safe, not for use under stream capture. */
int mgs_debug_set_blend_events(void* fwd_start, void* fwd_end, void* bwd_start, void* bwd_end);

/* TEST USE ONLY, process-global: 1 / 0 = the last blend backward launched by mgs_backward with blend_bwd_transposed = 2 walked
 * the lists split / unsplit; -1 = there was none yet. */
int mgs_debug_last_backward_split(void);
/* TEST USE ONLY, process-global: the number of 256-tile bands of the last render call's banded tile sort; 0 = it took the
 * two tile-sort passes.  The banded sort is the default on the per-tile path (mgs_binning_path() == 1, "pre_scan" on) when the
 * tile id is wider than 8 bits, the image has at most 32 bands of 256 tiles and the one pass's scratch fits the binning
 * scratch (it does from a few thousand instances up): the instances are emitted grouped by band from exact per-band counts
 * and ONE segmented 8-bit pass orders each band.  One more knob of mgs_debug_set_option switches it: "tile_sort_banded",
 * 1 = default, 0 = the plain emission and two passes everywhere; the same tables either way.  Set it between whole forwards,
 * like "pre_scan". */
int mgs_debug_last_tile_sort_bands(void);

/* TEST USE ONLY, a read-only window (pure apart from the options it follows, like mgs_binning_path; no launch, no device): the
 * route a forward of P Gaussians at W x H with cam.flags = `flags` takes, and -- for R instances, or with capacity_mode != 0 a
 * capacity of R -- the route of its render call, as MGS_PLAN_WORDS words in out[] [host].  One word per field of the forward
 * plan ("The forward plan"; csrc/forward_plan.h), flags as 0 / 1: */
enum {
    MGS_PLAN_P = 0, MGS_PLAN_W, MGS_PLAN_H, MGS_PLAN_FLAGS, MGS_PLAN_CAPACITY_MODE,           /* the inputs */
    MGS_PLAN_TILES_X, MGS_PLAN_TILES_Y, MGS_PLAN_NTILES, MGS_PLAN_TILE_BITS,
    MGS_PLAN_SMALL_GRID,       /* ntiles <= 65536 */
    MGS_PLAN_PER_TILE,         /* = mgs_binning_path(P, W, H) */
    MGS_PLAN_SCAN_ITEMS,       /* Gaussians per scan block: 256 = the per-Gaussian forward kernel scans ("pre_scan"), else 2048 */
    MGS_PLAN_SCAN_SHIFT, MGS_PLAN_SCAN_BLOCKS,
    MGS_PLAN_SCAN_SMALL,       /* the single-launch scan ("scan_small"; 2048-item granularity and at most 64 blocks only) */
    MGS_PLAN_BANDS_COUNTED,    /* bands of 256 tiles the preprocess half counts and scans ("tile_sort_banded"); 0 = none */
    MGS_PLAN_RECT_PACKED,      /* the depth sort carries packed rectangles (else its last pass gathers them) */
    MGS_PLAN_EXCLUSIVE,        /* MGS_FLAG_EXCLUSIVE_DEVICE */
    MGS_PLAN_R,                /* the render half from here: R, 0 when P == 0 */
    MGS_PLAN_R_CAP,            /* the emission's bound: the capacity; exact path 0xFFFFFFFF, or 0 when R == 0 */
    MGS_PLAN_SLOT_MAJOR,       /* emission balanced by output slots ("dup_slot_major") */
    MGS_PLAN_BANDS,            /* what mgs_debug_last_tile_sort_bands() reports after that render call */
    MGS_PLAN_COUNT_DIGITS,     /* the emission counts the tile sort's digits: no histogram launch */
    MGS_PLAN_KEY_SHIFT, MGS_PLAN_DEPTH_LO_BITS,       /* per-tile path: 32 - tile bits, depth bits kept in the value; else 0, 0 */
    MGS_PLAN_SORT_TILES,       /* per-tile path with R > 0: each tile's list is sorted by depth ... */
    MGS_PLAN_TILE_SORT_FUSED,  /* ... inside the blend forward ("tile_sort_fused"), else by a launch of its own */
    MGS_PLAN_DUP_THREADS,      /* threads of the plain emission's launch */
    MGS_PLAN_BANDED_BYTES,     /* scratch of the banded tile sort's one pass for R pairs (0 without counted bands) ... */
    MGS_PLAN_TWO_PASS_BYTES,   /* ... which must fit this, = mgs_debug_sort_temp_bytes(R, tile bits), for MGS_PLAN_BANDS != 0 */
    MGS_PLAN_WORDS
};
int mgs_debug_forward_plan(int32_t P, int32_t W, int32_t H, int32_t flags, uint64_t R, int32_t capacity_mode, uint64_t* out);

/* Diagnostic (not on the hot path): counts what the blend backward of the matching forward does, into
 * stats_dev[MGS_BLEND_STATS_WORDS] (device uint64): [0] 64-instance steps walked, [1] instances that pass the per-quadrant
 * cull and are fetched ("survivors"), [2] survivors with >= 1 active pixel (= wave reductions = atomic instructions),
 * [3] active (pixel, instance) pairs, [4] inactive survivors that are inactive only because of the depth order,
 * [5..7] active survivors with <= 2 / 4 / 8 active pixels.  bench.py divides the kernel's VALU instruction count
 * (rocprofv3 --pmc) by [1] and [2] to report instructions per survivor.
 * [8 + 3 d + {0, 1, 2}], d = 0..4 (round 5): what the walk would cost if the wave ran one survivor stream per GROUP of
 * pixels -- d = 0: two 8x4 halves (top / bottom), 1: two 4x8 halves (left / right), 2: four 4x4 blocks, 3: four 8x2 strips,
 * 4: eight 4x2 blocks -- with the cull run per group: {0} loop trips when the groups' survivor lists are paired step by step
 * (sum over steps of the longest group list), {1} (group, survivor) rows, {2} trips when every group runs down its own
 * list over the whole walk (sum over quadrant walks of the longest group total).  Compare with [1]. */
#define MGS_BLEND_STATS_WORDS 24
int mgs_debug_blend_stats(const mgs_camera* cam, int32_t P, uint64_t num_rendered, const void* geometry,
                          const void* binning, const void* image, uint64_t* stats_dev, void* stream);

/* Diagnostic (not on the hot path): the default blend backward (blend_backward_s_kernel) does not cull for itself, it walks the
 * survivor masks the blend forward left in the binning scratch.  This walks every quadrant's list as that backward does, back to
 * front, and counts into stats_dev[MGS_BLEND_MASK_STATS_WORDS] (device uint64): [0] 64-instance steps, [1] instances the
 * backward's own cull would keep (what mgs_debug_blend_stats calls survivors), [2] set bits of the forward's masks inside the
 * walked range (what the backward fetches and evaluates), [3] instances the own cull keeps and the forward's mask lacks: 0, or
 * the backward would lose contributions. */
#define MGS_BLEND_MASK_STATS_WORDS 4
int mgs_debug_blend_mask_stats(const mgs_camera* cam, int32_t P, uint64_t num_rendered, const void* geometry,
                               const void* binning, const void* image, uint64_t* stats_dev, void* stream);

/* ---- K-channel feature rendering (ABI v17) ---------------------------------------------------------------
 * Blends K arbitrary per-Gaussian channels (object probabilities, semantic logits, ...) through the lists and the per-pixel
 * decisions a finished forward left in its scratch, with the weights alpha T that forward's colours were blended with:
 *
 *     out[k, p] = sum_i features[g_i, k] alpha_i T_i  (+ final_T[p] bg[k] when bg is non-NULL)
 *
 * over the contributors i of pixel p -- list positions 1 .. n_contrib[p] with power <= 0 and alpha >= 1/255; the forward decided
 * where each pixel stops, nothing is re-decided here.  mgs_features_backward is the gradient to the features,
 *
 *     dL_dfeatures[g, k] = sum_p alpha T dL_dout[k, p],
 *
 * and the only one: bg, geometry, opacity and pose take none (the feature image is a read-out of a map the colour and depth
 * losses shape).  dL_dfeatures is cleared by the call; rows of Gaussians in no list stay exactly 0.
 *
 * LAYOUT: features and dL_dfeatures are [P, K] row-major, out and dL_dout [K, H, W], bg [K] (or NULL: no background term),
 * labels [H, W] int32 (or NULL).  K is 1 .. MGS_MAX_FEATURE_CHANNELS (segmentation ids are 8-bit in mgs_frame_prepare); K outside
 * that, or P > MGS_MAX_GAUSSIANS, returns 1.  labels[p] = the lowest index k that maximises the accumulated value WITHOUT the
 * background term, or -1 where 1.0f - final_T[p] < min_opacity (the float32 opacity the forward wrote).  P == 0: out = bg (or
 * 0), labels = -1, nothing else is read.
 * LIFETIME: `geometry`, `binning`, `image` are the scratch of a finished mgs_forward_render / _capacity for the same cam, P
 * and num_rendered (the capacity, in capacity mode: what mgs_backward takes); they are only READ, so the calls may come
 * before or after mgs_backward, any number of times, while the scratch is alive and unmodified.  Both functions keep no state
 * and never synchronise the host. */
#define MGS_MAX_FEATURE_CHANNELS 256
int mgs_features_forward(const mgs_camera* cam, int32_t P, int32_t K, uint64_t num_rendered, const void* geometry,
                         const void* binning, const void* image, const float* features /* [P,K] */,
                         const float* bg /* [K] or NULL */, float* out /* [K,H,W] */, int32_t* labels /* [H,W] or NULL */,
                         float min_opacity, void* stream);
int mgs_features_backward(const mgs_camera* cam, int32_t P, int32_t K, uint64_t num_rendered, const void* geometry,
                          const void* binning, const void* image, const float* dL_dout /* [K,H,W] */,
                          float* dL_dfeatures /* [P,K], cleared here */, void* stream);

/* ---- Pose-tangent rendering (ABI v29) ---------------------------------------------------------------------
 * The per-pixel Jacobian of the render with respect to the six pose tangents, tau = (rho_x, rho_y, rho_z, theta_x, theta_y,
 * theta_z) in the order of mgs_backward's dL_dtau, of T_cw(tau) = exp(tau^) T_cw at tau = 0: a forward-mode pass through the
 * lists and the per-pixel decisions a finished forward left in its scratch.
 *
 *     J[5 k + c, p] = d out_c[p] / d tau_k,   c = (R, G, B, depth, opacity),   J is [30, H, W] float32
 *
 * with the gradient conventions of mgs_backward: skip and termination decisions, radii and rectangles are constants, a
 * view-space ratio clamped at 1.3 tanfov is a constant, the 0.99 cap of alpha is straight-through.  Hence, for any cotangent
 * images (g_color, g_depth):  sum over p and c < 4 of g[c, p] J[5 k + c, p] = dL_dtau[k] of mgs_backward, to rounding.
 * A pixel with an empty list is exactly 0 in all 30 planes.  Opacities and colours are constants: only a forward that took
 * colors_precomp is supported (an SH colour depends on the camera position); after an `shs` forward (cam->sh_coeffs > 0) the
 * call returns 1.  means3D, scales / rotations or cov3D_precomp and radii are the forward's (what mgs_backward takes).
 * `tangent_scratch`: mgs_pose_tangent_bytes(P) bytes, written here (the per-Gaussian tangent records: 192 bytes each; the
 * records of Gaussians with radii == 0 are neither written nor read).
 * LIFETIME: as mgs_features_forward -- `geometry`, `binning`, `image` are the scratch of a finished mgs_forward_render /
 * _capacity for the same cam, P and num_rendered; they are only READ, on either binning path, before or after mgs_backward.
 * No host synchronisation, no state.  P == 0: J is cleared with one memset node, nothing else is read.  P > MGS_MAX_GAUSSIANS
 * or a NULL required pointer returns 1 before any launch. */
size_t mgs_pose_tangent_bytes(int32_t P);
int mgs_pose_jacobian(const mgs_camera* cam, int32_t P, uint64_t num_rendered, const float* means3D, const float* scales,
                      const float* rotations, const float* cov3D_precomp, const int32_t* radii, const void* geometry,
                      const void* binning, const void* image, void* tangent_scratch, float* J /* [30,H,W] */, void* stream);

/* ---- Surface depth: median depth, depth variance, depth normals (ABI v31) ------------------------------------
 * mgs_surface_depth: one more walk through the lists and the per-pixel decisions a finished forward left in its scratch
 * ("Surface depth").  For pixel p and its contributors i = 1 .. n in blend order -- list positions
 * 1 .. n_contrib[p] with power <= 0 and alpha >= 1/255, as mgs_features_forward -- with T_1 = 1, w_i = alpha_i T_i,
 * t_i = T_i (1 - alpha_i) = T_(i+1) and z_i the blend record's float32 view-space depth of the Gaussian's centre:
 *
 *     median_depth[p] = z_m, median_id[p] = the Gaussian's index, m = the first i with t_i <= 0.5;  0 and -1 if there is none
 *     depth_var[p]    = max(0, S2 / O - (S1 / O)^2),  O = sum w_i, S1 = sum w_i (z_i - z_1), S2 = sum w_i (z_i - z_1)^2;  0 for n = 0
 *
 * (m is the first contributor the forward did not count in n_touched).  Gates, on median_depth / median_id only: they become
 * 0 / -1 where 1.0f - final_T[p] < min_opacity (the float32 opacity the forward wrote), and where max_std > 0 and
 * depth_var[p] > max_std * max_std.  min_opacity = 0, max_std = 0 disables both.  `want`: which planes are written, a sum of the
 * bits below; median_id may be NULL.  max_std > 0 needs MGS_SURFACE_VARIANCE and its plane.  With MGS_SURFACE_MEDIAN alone and
 * max_std == 0 a wave leaves the walk once every pixel of its quadrant has its median or has passed its last contributor.
 * LIFETIME: as mgs_features_forward -- `geometry`, `binning`, `image` are the scratch of a finished mgs_forward_render /
 * _capacity for the same cam, P and num_rendered; they are only READ, on either binning path, before or after mgs_backward.
 * No atomics, no host synchronisation, no state: capturable, and bit-reproducible.  P == 0: the requested planes are cleared
 * (0, -1, 0), nothing else is read.  Returns 1 with a message before any launch for: a NULL plane that `want` asks for, want == 0
 * or unknown bits, a NaN or negative min_opacity / max_std, max_std > 0 without the variance, a NULL scratch pointer with P > 0.
 *
 * mgs_depth_normals: the camera-frame normal of a metric depth plane (d <= 0: invalid), central differences of the
 * back-projected pixel centres P(x, y) = d(x, y) ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1) -- the pixel centre of
 * mgs_backproject:
 *
 *     n = normalize((P(x+1, y) - P(x-1, y)) x (P(x, y+1) - P(x, y-1))),  negated if n . P(x, y) > 0 (it faces the camera)
 *
 * and (0, 0, 0) on the image border, where any of the five depths is invalid, where max_jump > 0 and a neighbour differs from the
 * centre depth by more than max_jump, and where the cross product has zero length.  normals is [3, H, W].  Plain IEEE float32
 * arithmetic in the order written above, no contraction.  W, H <= 0, W x H >= 2^31, a NULL pointer, non-finite or non-positive
 * fx / fy, a NaN cx / cy, a NaN or negative max_jump return 1 before any launch. */
#define MGS_SURFACE_MEDIAN   1   /* median_depth (and median_id if non-NULL) */
#define MGS_SURFACE_VARIANCE 2   /* depth_var */
int mgs_surface_depth(const mgs_camera* cam, int32_t P, uint64_t num_rendered, const void* geometry, const void* binning,
                      const void* image, int32_t want, float min_opacity, float max_std,
                      float* median_depth /* [H,W] */, int32_t* median_id /* [H,W] or NULL */, float* depth_var /* [H,W] */,
                      void* stream);
int mgs_depth_normals(int32_t W, int32_t H, const float* depth /* [H,W] */, float fx, float fy, float cx, float cy,
                      float max_jump, float* normals /* [3,H,W] */, void* stream);

/* ---- Label loss and confusion count of the object layer (ABI v21) ----------------------------------------
 * Softmax cross-entropy of a blended K-channel image against 8-bit ids, value + gradient to the image, for learning the
 * per-Gaussian object rows: feat is mgs_features_forward's `out` on the RAW rows (no background term), taken as logits, and
 * d_feat is what mgs_features_backward takes as dL_dout.
 *
 *     counted(p)   = (valid == NULL || valid[p] != 0) && labels[p] < K,    N = number of counted pixels
 *     L            = (1 / N) sum over counted p of [ logsumexp_k feat[k, p] - feat[labels[p], p] ]
 *     d_feat[k, p] = (softmax_k(feat[:, p]) - [k == labels[p]]) / N  on counted pixels, exactly 0 elsewhere
 *
 * N == 0: L = 0 and d_feat = 0, no NaN.  The softmax is max-subtracted: feat of +-1e4 stays finite.
 * LAYOUT: feat and d_feat [K, H, W] float32, labels and valid [H, W] bytes (valid may be NULL = every pixel), K is
 * 1 .. MGS_MAX_FEATURE_CHANNELS, width x height < 2^31.
 * mgs_label_prepare (once per keyframe: N depends on labels and valid alone) stores count_out[2] = {N, width x height - N} on
 * the device; mgs_label_loss_grads reads them there (`count`) and, in two launches, writes d_feat (every element, once) and
 * the loss, a float at scratch + MGS_LABEL_SCRATCH_LOSS.  `scratch`: mgs_label_scratch_bytes() bytes, 8-byte aligned, per
 * call; the two calls may share one.  Nothing is assumed of scratch, count_out or d_feat on entry and nothing is cleared:
 * every word read was stored by the same call (per-workgroup partial sums, added in a fixed order).  No atomics: loss and
 * gradient are bitwise reproducible from call to call.  No state is kept and the host is never synchronised.
 *
 * mgs_label_confusion ADDS into counts [K, K] uint32, indexed [gt, pred], one per counted pixel (the rule above, with gt as
 * labels) whose pred [H, W] int32 -- the `labels` of mgs_features_forward -- lies in 0 .. K-1, and into side[2] =
 * {counted pixels without such a prediction (-1 = not seen), pixels not counted}.  The caller clears counts and side before
 * the first call; integer atomics only, so the result is exact and independent of order.
 *
 * Bad arguments (K outside 1 .. MGS_MAX_FEATURE_CHANNELS, non-positive sizes, NULL required pointers, a misaligned scratch)
 * return 1 before anything is launched. */
#define MGS_LABEL_SCRATCH_LOSS 0
size_t mgs_label_scratch_bytes(void);
int mgs_label_prepare(int32_t width, int32_t height, int32_t K, const uint8_t* labels, const uint8_t* valid /* or NULL */,
                      void* scratch, uint32_t* count_out /* [2] */, void* stream);
int mgs_label_loss_grads(int32_t width, int32_t height, int32_t K, const float* feat /* [K,H,W] */, const uint8_t* labels,
                         const uint8_t* valid /* or NULL */, const uint32_t* count /* [2], of mgs_label_prepare */,
                         void* scratch, float* d_feat /* [K,H,W] */, void* stream);
int mgs_label_confusion(int32_t width, int32_t height, int32_t K, const int32_t* pred /* [H,W] */, const uint8_t* gt,
                        const uint8_t* valid /* or NULL */, uint32_t* counts /* [K,K], added to */,
                        uint32_t* side /* [2], added to */, void* stream);

/* ---- headless viewer (ABI v20) ---------------------------------------------------------------------------
 * What the reference's viewer window shows (viewer/slam_viewer.py: the shaders rgb / segmentation, depth, time, elipsoids and
 * the camera / trajectory line sets over them), as uint8 [H, W, 3] images on the device.  None of these calls synchronises the
 * host or keeps state; every clear is a kernel, so all of them may be captured in a hipGraph.
 *
 * mgs_viewer_ellipsoids: through the tables of a finished forward (LIFETIME as mgs_features_forward: `geometry`, `binning`,
 * `image` are only READ), out[:, p] = colour[g] exp(power) of the first entry g of pixel p's tile list, in blend order, with
 * power <= 0 and min(0.99, opacity exp(power)) > threshold; hit[p] = g (int32; hit may be NULL).  No such entry: black, -1.
 * The whole list is walked, whatever n_contrib says.  threshold must lie in [1/255, 1) (the viewer passes 0.4); P == 0: black.
 *
 * mgs_viewer_lines: segments [S, 4] int32 {x0, y0, x1, y1} in 1/16 pixel, pixel centres at multiples of 16, already clipped to
 * a guard rectangle by the caller.  Clears the owner image in `scratch` and rasterises with integer arithmetic only: along the
 * axis of the larger extent (x on a tie) every integer pixel position inside the segment, the other coordinate rounded half
 * up; a segment without such a position paints the pixel its first endpoint rounds to.  owner = highest segment index + 1.
 * Pixels outside the image are skipped.  S == 0 only clears.
 *
 * mgs_viewer_compose: out [H, W, 3] uint8 from the float image `src` by `mode`:
 *   MGS_VIEWER_RGB         src [3, H, W]: trunc(clip(c, 0, 1) * 255)                       (also the segmentation shader)
 *   MGS_VIEWER_DEPTH       src [H, W] >= 0: lut[jet index of src / max(src)], unnormalised when the maximum is 0; the maximum
 *                          is found on the device (`scratch`) and never read back
 *   MGS_VIEWER_TIME        src [H, W]: lut[jet index of src]                               (the reference shows the opacity image)
 *   MGS_VIEWER_ELLIPSOIDS  src [3, H, W]: floor(clip(c, 0, 1) * 255 + 0.5)                 (GL's unorm conversion)
 * jet index of x = clamp(floor(x * 256), 0, 255); a NaN gives black.  `lut` [256, 3] uint8 is needed by DEPTH and TIME.
 * n_segments > 0: the owner image a preceding mgs_viewer_lines left in the same `scratch` is resolved on top, pixel p with
 * owner k > 0 taking seg_rgb[k - 1] ([n_segments, 3] uint8); n_segments == 0: no overlay, the owner image is not read.
 * `scratch`: mgs_viewer_scratch_bytes(W, H) bytes, 256-byte aligned: the depth maximum's word at byte 0, the owner image
 * (int32 [H, W]) at byte 256.  Bad arguments (NULL pointers, an unknown mode, non-positive sizes) return 1 before any launch;
 * mgs_viewer_scratch_bytes returns 0 for them. */
#define MGS_VIEWER_RGB 0
#define MGS_VIEWER_DEPTH 1
#define MGS_VIEWER_TIME 2
#define MGS_VIEWER_ELLIPSOIDS 3
size_t mgs_viewer_scratch_bytes(int32_t W, int32_t H);
int mgs_viewer_ellipsoids(const mgs_camera* cam, int32_t P, uint64_t num_rendered, const void* geometry, const void* binning,
                          const void* image, float threshold, float* out /* [3,H,W] */, int32_t* hit /* [H,W] or NULL */,
                          void* stream);
int mgs_viewer_lines(int32_t W, int32_t H, const int32_t* segments /* [S,4] */, int32_t n_segments, void* scratch, void* stream);
int mgs_viewer_compose(int32_t mode, int32_t W, int32_t H, const float* src, const uint8_t* lut /* [256,3] */,
                       const uint8_t* seg_rgb /* [S,3] */, int32_t n_segments, void* scratch, uint8_t* out /* [H,W,3] */,
                       void* stream);

/* visible[P] (1 byte each) = view-space z > 0.2 (upstream markVisible; unused by MonoGS). */
int mgs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* visible, void* stream);

/* out[P] = mean squared distance to the 3 nearest other points (exact). */
size_t mgs_knn_scratch_bytes(int32_t P);
int mgs_dist2_knn(int32_t P, const float* points /* [P,3] */, float* out /* [P] */,
                  void* scratch, void* stream);

/* ---- Fused SLAM losses (caller-side widening) --------------------------------
 * Forward value + analytic gradients of get_loss_mapping (/root/reference/utils/slam_utils.py:101-146,
 * mode = 0) and get_loss_tracking (:58-98, mode & MGS_LOSS_TRACKING).  MGS_LOSS_INVERT_DEPTH selects the reference's
 * `invert_depth=True` branch (:83-88, :138-141): the depth term compares 1 / (depth + eps) with 1 / (gt_depth + eps),
 * eps = 1e-6 in the tracking loss and 0 in the mapping loss, exactly as the reference writes the two.  render[3,H,W], depth[1,H,W], opacity[1,H,W]
 * (tracking only), gt_rgb[3,H,W], gt_depth[H,W]; mask / grad_mask are [H,W] bytes (0 / non-zero; mask may be
 * NULL = all ones); exposure_a / exposure_b are device scalars (ignored when init != 0: rgb = render).
 * mgs_loss_forward writes the scalar loss to loss_out [device] and keeps its sums in `scratch`
 * (mgs_loss_scratch_bytes); mgs_loss_backward turns them into d_render[3,H,W], d_depth[1,H,W] and
 * d_exposure[2] = (dL/da, dL/db; may be NULL), all scaled by the device scalar grad_out (NULL = 1).
 * The opacity image gets no gradient (the rasteriser ignores dL/dopacity).
 * d_exposure is STORED (scale x the unscaled sums the forward kept in its per-workgroup partials: no atomics, no clear,
 * bitwise reproducible); it may be the two floats at scratch + MGS_LOSS_SCRATCH_DAB.
 * MGS_LOSS_RGB_ONLY (ABI v19; monocular frames, a [RECALL] of upstream MonoGS' get_loss_tracking_rgb / get_loss_mapping_rgb):
 * the depth term is dropped and with it its images -- depth, gt_depth and d_depth may be NULL and are never read; a non-NULL
 * d_depth is zero-filled (a memset node).  Tracking: L = 0.5 mean(opacity) mean_{3HW}(m |rgb - gt|), m = mask grad_mask
 * (opacity > 0.99).  Mapping: L = mean_{mask, 3 ch} |rgb - gt|; lambda_rgb is ignored (coefficient 1).  The colour sums are
 * formed exactly as without the bit: the results equal, bit for bit, the tracking mode on gt_depth = 0 and the mapping mode
 * on lambda_rgb = 1 with an all-positive gt_depth.  MGS_LOSS_INVERT_DEPTH has nothing to act on then and is ignored. */
#define MGS_LOSS_TRACKING 1
#define MGS_LOSS_INVERT_DEPTH 2
#define MGS_LOSS_RGB_ONLY 4
#define MGS_LOSS_SCRATCH_DAB 10
#define MGS_LOSS_SCRATCH_LOSS 12
size_t mgs_loss_scratch_bytes(void);
int mgs_loss_forward(int32_t width, int32_t height, int32_t mode, int32_t init, float lambda_rgb,
                     const float* render, const float* depth, const float* opacity, const float* gt_rgb,
                     const float* gt_depth, const uint8_t* mask, const uint8_t* grad_mask,
                     const float* exposure_a, const float* exposure_b, float* scratch, float* loss_out,
                     void* stream);
int mgs_loss_backward(int32_t width, int32_t height, int32_t mode, int32_t init, float lambda_rgb,
                      const float* render, const float* depth, const float* opacity, const float* gt_rgb,
                      const float* gt_depth, const uint8_t* mask, const uint8_t* grad_mask,
                      const float* exposure_a, const float* exposure_b, const float* scratch,
                      const float* grad_out, float* d_render, float* d_depth, float* d_exposure, void* stream);
/* Loss value AND gradients (for grad_out = 1) in two launches, for loops that drive the rasteriser's backward themselves
 * (torch.autograd.backward([color, depth], [d_render, d_depth])) instead of building an autograd node for the scalar:
 * no finalize kernel, no ones-fill.  Afterwards scratch[MGS_LOSS_SCRATCH_LOSS] holds the loss value and
 * scratch[MGS_LOSS_SCRATCH_DAB .. +1] hold dL/d(exposure_a), dL/d(exposure_b) (unless `init`). */
int mgs_loss_grads(int32_t width, int32_t height, int32_t mode, int32_t init, float lambda_rgb,
                   const float* render, const float* depth, const float* opacity, const float* gt_rgb,
                   const float* gt_depth, const uint8_t* mask, const uint8_t* grad_mask,
                   const float* exposure_a, const float* exposure_b, float* scratch, float* d_render, float* d_depth,
                   void* stream);

/* ---- Fused SSIM and the colour-refinement loss (the `fused_ssim` drop-in) ---------------------------------
 * SSIM of Wang et al. 2004 as 3DGS code bases use it: per plane (one channel of one image; img1 / img2 are
 * [planes,H,W] float32), the normalised 11-tap Gaussian window of sigma 1.5 applied separably with zero padding, mean of
 * the map over all pixels (valid = 0, padding "same") or over the map without its outer 5 pixels (valid != 0, padding
 * "valid"; needs width, height >= 11).  C1 / C2 are the two stabilising constants (MGS_SSIM_C1 / MGS_SSIM_C2 upstream).
 * mgs_ssim_forward writes the mean to value_out [device scalar]; with train != 0 it also leaves the three derivative
 * planes of the map in `scratch` (mgs_ssim_scratch_bytes, same planes / size / train), from which mgs_ssim_backward forms
 * d_img1[planes,H,W] = grad_out x d(mean)/d(img1) (grad_out: device scalar, NULL = 1).  img2 gets no gradient.
 * No atomics: per-workgroup partial sums added in a fixed order, values bitwise reproducible.
 *
 * Refinement loss (/root/reference/utils/slam_mapper.py:529-539): L = (1 - lambda) mean|render - gt| + lambda (1 - SSIM_valid),
 * render / gt_rgb [3,H,W].  mgs_refine_loss_forward / _backward are the two halves for an autograd node (loss_out, grad_out:
 * device scalars); mgs_refine_loss_grads gives the value AND d_render for grad_out = 1 with no host synchronisation.  After
 * any of the forwards scratch[MGS_SSIM_SCRATCH_LOSS], [.._L1], [.._SSIM] hold the loss, the L1 mean and the SSIM
 * (scratch: mgs_ssim_scratch_bytes(3, width, height, 1)). */
#define MGS_SSIM_C1 0.0001f
#define MGS_SSIM_C2 0.0009f
#define MGS_SSIM_SCRATCH_LOSS 0
#define MGS_SSIM_SCRATCH_L1 1
#define MGS_SSIM_SCRATCH_SSIM 2
size_t mgs_ssim_scratch_bytes(int32_t planes, int32_t width, int32_t height, int32_t train);
int mgs_ssim_forward(int32_t planes, int32_t width, int32_t height, int32_t valid, int32_t train, float C1, float C2,
                     const float* img1, const float* img2, float* scratch, float* value_out, void* stream);
int mgs_ssim_backward(int32_t planes, int32_t width, int32_t height, int32_t valid, float C1, float C2,
                      const float* img1, const float* img2, const float* scratch, const float* grad_out,
                      float* d_img1, void* stream);
int mgs_refine_loss_forward(int32_t width, int32_t height, float lambda_ssim, const float* render, const float* gt_rgb,
                            float* scratch, float* loss_out, void* stream);
int mgs_refine_loss_backward(int32_t width, int32_t height, float lambda_ssim, const float* render, const float* gt_rgb,
                             const float* scratch, const float* grad_out, float* d_render, void* stream);
int mgs_refine_loss_grads(int32_t width, int32_t height, float lambda_ssim, const float* render, const float* gt_rgb,
                          float* scratch, float* d_render, void* stream);

/* ---- Fused pose update (caller-side widening) -------------------------------
 * torch.optim.Adam.step() on (cam_rot_delta lr_rot, cam_trans_delta lr_trans, exposure_a/b lr_exposure)
 * followed by update_pose (/root/reference/utils/pose_utils.py:76-93): T_cw <- exp([rho; theta]^) T_cw,
 * deltas reset to zero.  R[3,3] (row-major), T[3], the parameters and the Adam moments adam_m[8], adam_v[8]
 * (order rot(3), trans(3), a, b) are device tensors updated in place; `step` is the 1-based Adam step, or, when
 * step_counter (device int32) is non-NULL, the counter is incremented on the device and used instead (so the call
 * can be captured in a hipGraph and replayed);
 * out[2] = {converged (|tau| < converged_threshold ? 1 : 0), |tau|}.  exposure pointers / any gradient may be NULL.
 * flags: MGS_POSE_STICKY makes the call a no-op once out[0] reports convergence (the tracker's early exit,
 * /root/reference/utils/slam_tracker.py:172-176, for loops replayed from a hipGraph); zero out[] to start over.
 * Camera refresh (optional, all four or none): with viewmatrix / projmatrix / campos non-NULL the kernel also recomputes
 * the viewpoint's camera tensors from the NEW R, T and projmatrix_raw -- bit-identical to mgs_camera_setup -- so the next
 * render of the loop needs no camera launch of its own. */
#define MGS_POSE_STICKY 1
int mgs_pose_step(float* R, float* T, float* rot_delta, float* trans_delta, float* exposure_a, float* exposure_b,
                  const float* grad_rot, const float* grad_trans, const float* grad_a, const float* grad_b,
                  float* adam_m, float* adam_v, int32_t step, float lr_rot, float lr_trans, float lr_exposure,
                  float beta1, float beta2, float eps, float converged_threshold, int32_t* step_counter, float* out,
                  int32_t flags, float* host_flag /* optional: pinned host word that also receives out[0] */,
                  const float* projmatrix_raw, float* viewmatrix, float* projmatrix, float* campos /* optional refresh */,
                  void* stream);
/* The same update for n <= 16 independent viewpoints in ONE launch (the keyframes of a mapping window,
 * /root/reference/utils/slam_mapper.py:486-496).  `ptrs`: HOST array of n x 18 device pointers in the order of mgs_pose_step's
 * pointer arguments (R, T, rot_delta, trans_delta, exposure_a, exposure_b, grad_rot, grad_trans, grad_a, grad_b, adam_m, adam_v,
 * step_counter [required], out, projmatrix_raw, viewmatrix, projmatrix, campos; NULL where optional); the scalars are shared. */
int mgs_pose_step_batch(int32_t n, void* const* ptrs, float lr_rot, float lr_trans, float lr_exposure, float beta1,
                        float beta2, float eps, float converged_threshold, int32_t flags, void* stream);

/* ---- Gauss-Newton tracking (ABI v29) ------------------------------------------------------------------------
 * mgs_gn_normal_equations: the normal equations of the tracking loss's rows in the unknowns x = (rho, theta, a, b), from the
 * planes J of mgs_pose_jacobian and the images mgs_loss_* takes in MGS_LOSS_TRACKING mode:
 *
 *     colour  r_c = e^a C_c + b - I_c   where mask grad_mask (O > 0.99)   d r / d x = (e^a J[5 k + c], e^a C_c, 1)   s = 0.5 / (3 H W)
 *     depth   r_d = D - D_gt            where (D_gt > 0) (O > 0.99)        d r / d x = (J[5 k + 3], 0, 0)             s = 1 / N_d
 *
 *     H = sum s omega j j^T,   g = sum s omega r j,   E = sum s huber(r),   omega = 1 if |r| <= delta else delta / |r|
 *
 * omega is formed in float32 (delta_rgb for colour rows, delta_depth, in the depth's unit, for depth rows); every product and
 * sum is carried in double.  The reference's factor mean(O) is dropped.  MGS_LOSS_RGB_ONLY drops the depth rows and their
 * images (depth, gt_depth may be NULL).  exposure_a / exposure_b NULL (both): a = b = 0.  mask may be NULL (all ones).
 * `system` [MGS_GN_SYSTEM_DOUBLES] device doubles: H[8][8] row-major (symmetric, full), g[8], E, N_rgb (pixels with colour
 * rows), N_d.  N_d == 0 or an all-masked frame gives zeros, never NaN.  `scratch`: mgs_gn_scratch_bytes(width, height), 8-byte
 * aligned.  Two launches, no atomics, partial sums added in a fixed order: bitwise reproducible.
 *
 * mgs_pose_gn_step: one wave solves (H + lam diag(H) + lam_abs I) x = -g by Cholesky in double -- with MGS_GN_FIX_EXPOSURE (or
 * NULL exposure pointers) the 6 x 6 pose block --, scales the whole step so that |theta| <= max_rot and |rho| <= max_trans,
 * retracts T_cw <- exp([rho; theta]^) T_cw exactly as mgs_pose_step does, adds x[6], x[7] to the exposure, and (optional, all
 * four or none) refreshes the camera tensors bit-identically to mgs_camera_setup.
 * out[4] = {converged (|tau| < converged_threshold), |tau|, E, status}; host_flag (optional, pinned) receives out[0].
 * A non-positive or non-finite pivot: no update, status = 1, R, T, a, b bit-unchanged.  MGS_POSE_STICKY as for mgs_pose_step. */
#define MGS_GN_SYSTEM_DOUBLES 75
#define MGS_GN_FIX_EXPOSURE 2
size_t mgs_gn_scratch_bytes(int32_t width, int32_t height);
int mgs_gn_normal_equations(int32_t width, int32_t height, int32_t mode, const float* J /* [30,H,W] */, const float* render,
                            const float* depth, const float* opacity, const float* gt_rgb, const float* gt_depth,
                            const uint8_t* mask, const uint8_t* grad_mask, const float* exposure_a, const float* exposure_b,
                            float delta_rgb, float delta_depth, void* scratch, double* system, void* stream);
int mgs_pose_gn_step(float* R, float* T, float* exposure_a, float* exposure_b, const double* system, float lam, float lam_abs,
                     float max_rot, float max_trans, float converged_threshold, float* out /* [4] */, int32_t flags,
                     float* host_flag, const float* projmatrix_raw, float* viewmatrix, float* projmatrix, float* campos,
                     void* stream);

/* ---- Keyframe back-projection ------------------------------------------------
 * The per-point part of GaussianModel.create_viewpoint_pcd (/root/reference/gaussian_splatting/scene/gaussian_model.py:121-319)
 * for N selected pixels: gather rgb (with the tracked exposure exp(a)*rgb + b clamped to [0,1] when exposure_a is
 * non-NULL) and depth, unproject the pixel centre (x+0.5, y+0.5) with (fx, fy, cx, cy) and move it to the world
 * with the world->camera pose (R row-major, T): p_w = R^T (p_c - T).  selected[i] = x * H + y (the reference's
 * flattening order, gaussian_model.py:180-187).  segmentation / ids may be NULL. */
int mgs_backproject(int32_t N, int32_t W, int32_t H, const int64_t* selected, const float* rgb /* [3,H,W] */,
                    const float* depth /* [H,W] */, const int32_t* segmentation /* [H,W] or NULL */,
                    const float* exposure_a, const float* exposure_b, float fx, float fy, float cx, float cy,
                    const float* R, const float* T, float* points /* [N,3] */, float* features /* [N,3] */,
                    int32_t* ids /* [N] or NULL */, void* stream);

/* ---- Camera matrices of one viewpoint ---------------------------------
 * From the world->camera rotation R[3,3] (row-major) and translation T[3] and the transposed projection
 * projmatrix_raw[4,4]: viewmatrix = getWorld2View(R, T)^T (/root/reference/gaussian_splatting/utils/graphics_utils.py:33-42,
 * /root/reference/utils/camera_utils.py:171-174), projmatrix = viewmatrix @ projmatrix_raw
 * (/root/reference/utils/camera_utils.py:224-231), campos = viewmatrix^-1[3,:3] = -R^T T
 * (/root/reference/utils/camera_utils.py:176-178).  One launch; all pointers are device memory. */
int mgs_camera_setup(const float* R, const float* T, const float* projmatrix_raw, float* viewmatrix /* [16] */,
                     float* projmatrix /* [16] */, float* campos /* [3] */, void* stream);

/* ---- Fused Gaussian optimiser step + densification statistics ---------------
 * mgs_adam_step: torch.optim.Adam defaults over n_tensors <= 8 float tensors in one launch (the reference's five
 * groups: /root/reference/gaussian_splatting/scene/gaussian_model.py:398-442).  All tables are HOST arrays of
 * device pointers / sizes / learning rates; grads[t] may be NULL: that tensor is skipped (parameter, moments and step
 * count untouched), as torch.optim.Adam skips a parameter whose .grad is None.  `step` is the 1-based step, or
 * step_counter (device int32[n_tensors], one count per tensor like torch's state["step"]) is incremented on the
 * device for the tensors that have a gradient and used instead (hipGraph-capturable).
 * mgs_densify_stats: for the Gaussians with radii > 0,  xyz_gradient_accum += ||viewspace_grad[:, :2]||,
 * denom += 1 (gaussian_model.py:888-892), max_radii_2d = max(max_radii_2d, radii) (utils/slam_mapper.py:453-457);
 * any of the three outputs may be NULL. */
int mgs_adam_step(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const uint64_t* numel, const float* lr, double beta1, double beta2,
                  double eps, int32_t step, int32_t* step_counter,
                  const float* lr_device /* device float[n_tensors] used instead of lr[] when non-NULL: a schedule
                                            stepped on the device (mgs_lr_schedule_step), hipGraph-replayable */,
                  void* stream);
int mgs_densify_stats(int32_t P, const float* viewspace_grad /* [P,3] */, const int32_t* radii,
                      float* xyz_gradient_accum /* [P] */, float* denom /* [P] */, float* max_radii_2d /* [P] */,
                      void* stream);
/* The statistics of ONE mapping iteration over the n_keyframes <= 32 keyframes a rank rendered, in one launch -- what
 * /root/reference/utils/slam_mapper.py:400-404,453-460 does keyframe by keyframe after loss.backward():
 *   visibility_bits[k][w] bit i = (n_touched_k[64 w + i] > 0)   (occ_aware_visibility; uint64 words, ceil(P/64) per keyframe;
 *                                                                 may be NULL)
 *   over v = radii_k > 0:  grad_norm[v] += ||grad_means2D_k[v, :2]||,  visible[v] += 1,  max_radii[v] = max(., radii_k[v])
 * The keyframe tables are HOST arrays of device pointers (grad_means2D[k] may be NULL).  accumulate != 0: the three arrays
 * are the map's running statistics (xyz_gradient_accum, denom, max_radii_2d) and end up bit for bit as the reference's
 * loop over keyframes leaves them; accumulate == 0 (keyframe-sharded window): they receive this rank's share of the
 * iteration only, to be summed / maximised across ranks and folded in with mgs_window_apply. */
int mgs_window_stats(int32_t P, int32_t n_keyframes, const float* const* grad_means2D, const int32_t* const* radii,
                     const int32_t* const* n_touched, float* grad_norm /* [P] */, float* visible /* [P] */,
                     float* max_radii /* [P] */, int32_t accumulate, uint64_t* visibility_bits, void* stream);
int mgs_window_apply(int32_t P, const float* grad_norm, const float* visible, const float* max_radii,
                     float* xyz_gradient_accum, float* denom, float* max_radii_2d, void* stream);
/* GaussianModel.update_learning_rate (/root/reference/gaussian_splatting/scene/gaussian_model.py:451-465, schedule
 * /root/reference/gaussian_splatting/utils/general_utils.py:79-94) on the device: *iteration += 1, *lr_out = schedule of
 * the new value -- the mapper's `self.nr_iters` and the xyz group's learning rate, kept in device memory so that a
 * captured mapping iteration steps them itself. */
int mgs_lr_schedule_step(int32_t* iteration, float* lr_out, double lr_init, double lr_final, int32_t lr_delay_steps,
                         double lr_delay_mult, int32_t max_steps, void* stream);

/* ---- Fused map activations ------------------------------------------------
 * rotations = F.normalize(rot_raw), scales3 = exp(scale_raw) (isotropic [P,1] expanded to [P,3] as render() does),
 * opacities = sigmoid(opacity_raw): /root/reference/gaussian_splatting/scene/gaussian_model.py:84-106 and
 * gaussian_renderer/__init__.py:101-104.  One launch forward, one backward (any gradient / output may be NULL). */
int mgs_activate_forward(int32_t P, int32_t scale_dim /* 1 or 3 */, const float* rot_raw /* [P,4] */,
                         const float* scale_raw /* [P,scale_dim] */, const float* opacity_raw /* [P] */,
                         float* rotations /* [P,4] */, float* scales3 /* [P,3] */, float* opacities /* [P] */,
                         void* stream);
int mgs_activate_backward(int32_t P, int32_t scale_dim, const float* rot_raw, const float* scales3,
                          const float* opacities, const float* grad_rotations, const float* grad_scales3,
                          const float* grad_opacities, float* d_rot_raw, float* d_scale_raw, float* d_opacity_raw,
                          void* stream);

/* dst[i] = src_0[i] + src_1[i] + ... (1..16 device buffers of `count` floats, `src` a HOST array of device pointers; dst may
 * be one of the sources): the gradients that the N keyframe renders of a mapping window return for the same map tensor,
 * summed in ONE launch instead of the autograd engine's N - 1 pairwise adds per tensor (monogs_amd.window.fan_out). */
int mgs_sum_buffers(int32_t n_src, const float* const* src, float* dst, uint64_t count, void* stream);

/* ---- Keyframe selection and window management on the device (ABI v14) ----------------------------------------
 * The three quantities /root/reference/utils/slam_tracker.py:192-284,412-452 decides from, and the decision, without a host
 * synchronisation: every call is stream-ordered, keeps no state between calls, assumes nothing about the contents of its
 * scratch or outputs on entry and can be captured in a hipGraph.  Counting is integer only: results are bitwise reproducible.
 *
 * mgs_masked_median: get_median_depth(depth, mask) (/root/reference/utils/slam_utils.py:149-157) with a free lower bound.
 *   Element i counts when values[i] > lo and (mask == NULL or mask[i] != 0); mask is a FLOAT array (the reference passes the
 *   opacity image to logical_and).  With c counted elements *out_median is the one of ascending rank (c - 1) / 2 -- torch's
 *   lower median -- and *out_count = c.  c == 0 (n == 0 included) writes NaN and 0; the reference's torch.median raises on
 *   an empty tensor instead.  Exact radix select on an order-preserving 32-bit key (any finite floats, lo = -inf allowed),
 *   three digit passes, six launches whatever the data.  NaN values are out of contract; 0 <= n < 2^32.
 *   scratch: mgs_median_scratch_bytes(n) bytes of device memory (a pure function of n, monotone).
 * mgs_covisibility: counts[k] = { |A and B_k|, |A or B_k|, |A|, |B_k| } (uint32[K][4]) for the current frame's set A and the
 *   K <= 32 window keyframes' sets B_k.  A is given as EXACTLY ONE of cur_n_touched (int32[P], packed on the fly as > 0) and
 *   cur_bits (ceil(P/64) words); the rows have the layout of mgs_window_stats' visibility_bits.  kf_bits / kf_words are HOST
 *   arrays of K device pointers / row lengths in words: a row shorter than ceil(P/64) words is zero-extended (the map grew
 *   since it was written), bits at or beyond P never count.  cur_bits_out (optional, ceil(P/64) words) receives the packed
 *   current row with a zero tail, ready to be kept as that frame's row if it becomes a keyframe.  K == 0 or P == 0 returns 0
 *   without a launch.  One memset node + one launch.
 * mgs_keyframe_decide: one wave.  poses: HOST array of 2 (K + 1) device pointers R[3,3] (row-major), T[3] (world->camera),
 *   the current frame first, then the K window keyframes, most recent first; counts as mgs_covisibility writes them for the
 *   same order; median: device float (mgs_masked_median's result).  With t(.) the translation of a 4x4 matrix:
 *     IoU = |A and B_0| / |A or B_0| (float32),  d = || t(T_cur T_0^-1) ||
 *     create = !check_overlap ? true : K < window_size ? IoU < kf_overlap
 *              : (IoU < kf_overlap && d > kf_min_translation * median) || d > kf_translation * median
 *     create_kf = create && frames_since_last_kf >= kf_interval
 *   Eviction is computed as if the frame were added: new list = [cur] + window.  For the positions i >= n_dont_touch,
 *   r_i = |A and B_i| / min(|A|, |B_i|); every r_i <= (window_full ? kf_cutoff : 0.4) is a candidate and only the LAST one
 *   (largest i) is removed.  If the list is then still longer than window_size, of the remaining i >= n_dont_touch the first
 *   maximum of  sqrt(|| t(T_i T_cur^-1) ||) * sum_{j >= n_dont_touch, j != i} 1 / (|| t(T_i T_j^-1) || + 1e-6)  is removed.
 *   A zero denominator gives NaN, NaN compares false: nothing is created or removed by it.
 *   out[8] (uint32) = { create_kf, removed_by_cutoff, removed_by_size, IoU bits, d bits, median bits, 0, 0 }; the removed
 *   slots are positions in the new list, (uint32)-1 = none.  1 <= K <= 32, window_size >= 1, n_dont_touch >= 1.
 * Argument errors of all three return 1 with a message, before anything is launched. */
typedef struct MgsKeyframeParams {
    int32_t K;                     /* keyframes in the window */
    int32_t window_size;
    int32_t window_full;           /* the tracker's is_window_full */
    int32_t check_overlap;         /* check_viewpoints_overlap */
    int32_t kf_interval;
    int32_t frames_since_last_kf;  /* cur_frame_idx - last_keyframe_idx */
    float kf_translation;          /* 0.08 */
    float kf_min_translation;      /* 0.05 */
    float kf_overlap;              /* 0.9 */
    float kf_cutoff;
    int32_t n_dont_touch;          /* 2 */
} MgsKeyframeParams;
size_t mgs_median_scratch_bytes(uint64_t n);
int mgs_masked_median(const float* values, const float* mask /* [n] or NULL */, uint64_t n, float lo, void* scratch,
                      float* out_median, uint32_t* out_count, void* stream);
int mgs_covisibility(int32_t P, const int32_t* cur_n_touched, const uint64_t* cur_bits, int32_t K,
                     const uint64_t* const* kf_bits, const uint64_t* kf_words, uint64_t* cur_bits_out,
                     uint32_t* counts /* [K][4] */, void* stream);
int mgs_keyframe_decide(const MgsKeyframeParams* params, const uint32_t* counts, const float* median,
                        const float* const* poses, uint32_t* out /* [8] */, void* stream);

/* ---- Depth hypothesis of a keyframe without measured depth (ABI v19) ------------------------------------------------
 * Monocular operation: the image the back-projection reads in place of a sensor's depth, from the keyframe's frozen render.
 * A [RECALL] of public upstream MonoGS' add_new_keyframe, anchored on what the reference keeps of it
 * (get_median_depth(..., return_std=True), /root/reference/utils/slam_utils.py:149-157; rgb_boundary_threshold in every config):
 * parity unpinned.  One stream-ordered call, no host read-back, no state between calls, capturable in a hipGraph.
 *   valid   = render_depth > 0 && render_opacity > opacity_min && valid_rgb      (a NULL image passes its test everywhere)
 *   median  = lower median of render_depth[valid] (mgs_masked_median);  std = its UNBIASED standard deviation (torch.std),
 *             two passes -- mean, then squared deviations -- over per-workgroup double-precision partials added in a fixed
 *             order: no float atomics, bitwise reproducible;  count = |valid|
 *   outlier = render_depth > median + std || render_depth < median - std || !valid      (both sums rounded to float32)
 *   depth_out = (outlier ? median : render_depth) + noise * (outlier ? sigma_out : sigma_in) * std
 *   init rule -- render_depth == NULL, or count < 2 (std undefined): depth_out = init_mean + init_sigma * noise
 *   depth_out = 0 exactly where valid_rgb is 0, under either rule.
 * noise: [H,W] standard normals the caller draws (no generator in the kernel).  stats_out[4] (device floats) = { median, std,
 * count, used_init_rule (0 / 1) }; under the init rule the first two hold init_mean and init_sigma.  render_opacity is ignored
 * without render_depth.  scratch: mgs_pseudo_depth_scratch_bytes(W x H) bytes, 256-byte aligned (may be NULL without
 * render_depth); nothing is assumed about its contents.  Nine launches with a render, one without; the elementwise kernels
 * read 4-pixel vectors when W x H % 4 == 0 and the images are 16-byte (valid_rgb: 4-byte) aligned, else pixel by pixel.
 * W x H < 2^32.  Argument errors return 1 with a message before anything is launched. */
typedef struct MgsPseudoDepthParams {
    float init_mean;       /* 2.0 */
    float init_sigma;      /* 0.3 */
    float opacity_min;     /* 0.95 */
    float sigma_in;        /* 0.2 */
    float sigma_out;       /* 0.5 */
} MgsPseudoDepthParams;
size_t mgs_pseudo_depth_scratch_bytes(uint64_t n);
int mgs_pseudo_depth(int32_t width, int32_t height, const float* render_depth /* [H,W] or NULL: init rule */,
                     const float* render_opacity /* [H,W] or NULL */, const uint8_t* valid_rgb /* [H,W] or NULL */,
                     const float* noise /* [H,W] */, const MgsPseudoDepthParams* params, void* scratch,
                     float* depth_out /* [H,W] */, float* stats_out /* [4] */, void* stream);

/* ---- Image metrics of a rendered frame (ABI v15) -------------------------------------------------------------
 * What eval_rendering (/root/reference/utils/eval_utils.py:169-183) computes per evaluated frame, in ONE pass over the render
 * and its ground truth (both [3,H,W]) and a one-workgroup finalize:
 *   clamped_out = clamp(render, 0, 1)                                         (:169)
 *   u8_out[y][x][c] = (uint8)(clamped_out[c][y][x] * 255.0f), a truncation    (:172; [H,W,3], may be NULL)
 *   over the elements with gt > 0, elementwise over the three planes (:180-182): mse = mean (clamped_out - gt)^2,
 *   psnr = 20 log10(1 / sqrt(mse))   (/root/reference/gaussian_splatting/utils/image_utils.py:19-21)
 *   row_out (device float[4]) = { psnr, <not touched>, mse, count }
 * Slot 1 is the caller's: the SSIM of :183 is mgs_ssim_forward(3, width, height, 1, 0, MGS_SSIM_C1, MGS_SSIM_C2, clamped_out,
 * gt, ..., row_out + 1) on the same stream.  count == 0 writes NaN for mse and psnr (the mgs_masked_median convention; the
 * reference's mean of an empty tensor is NaN as well); mse == 0 gives psnr = +inf.  The sums are carried in double through
 * per-workgroup partials added in a fixed order: no atomics, no clear launch, bitwise reproducible, mse within 1e-6 relative of
 * a float64 evaluation; count is exact (stored as float: up to 2^24 elements).  16-byte accesses when the three float bases
 * are 16-byte aligned, u8_out 4-byte aligned and width x height a multiple of 4, a scalar path otherwise.
 * scratch: mgs_metrics_scratch_bytes(width, height) bytes, 8-byte aligned, contents irrelevant on entry.
 * A NULL pointer (other than u8_out), width < 1 or height < 1 returns 1 with a message, before anything is launched;
 * 3 x width x height must stay below 2^31. */
size_t mgs_metrics_scratch_bytes(int32_t width, int32_t height);
int mgs_image_metrics(int32_t width, int32_t height, const float* render /* [3,H,W] */, const float* gt /* [3,H,W] */,
                      float* clamped_out /* [3,H,W] */, uint8_t* u8_out /* [H,W,3] or NULL */, void* scratch,
                      float* row_out /* device float[4] */, void* stream);

/* ---- Frame ingest: from a decoded frame to what the tracker is handed (ABI v16) --------------------------------
 * What MonocularDataset.__getitem__ (/root/reference/utils/dataset.py:410-508) and CameraExtrinsics.compute_grad_mask
 * (/root/reference/utils/camera_utils.py:184-212 with utils/slam_utils.py:6-40) do per frame, stream-ordered on the caller's
 * stream: no host synchronisation, no state between calls, nothing assumed about the contents of scratch or outputs on entry,
 * capturable in a hipGraph as a linear chain of kernel nodes.
 *
 * mgs_grad_mask: compute_grad_mask of a float [3,H,W] image on the device.
 *   gray = (r + g + b) / 3                                                                  (camera_utils.py:187)
 *   gv, gh = the Scharr responses [[3,10,3],[0,0,0],[-3,-10,-3]] and [[3,0,-3],[10,0,-10],[3,0,-3]] of the grey image
 *            reflect-padded by one pixel, both times 1/32                                   (slam_utils.py:6-23)
 *   valid  = all nine padded neighbours have |gray| > eps                                   (slam_utils.py:26-40)
 *   intensity = sqrt((gv valid)^2 + (gh valid)^2)  -> intensity_out (float [H,W], may be NULL)     (:190-192)
 *   grad_mask_out (uint8 [H,W], 0/1) = intensity > __fmul_rn(median, edge_threshold), median the LOWER median of all
 *            H W intensities (torch.median), found by mgs_masked_median with lo = -inf and no mask   (:211-212)
 *   The reference fixes edge_threshold = 1.1 (MGS_EDGE_THRESHOLD) and eps = 0.01 (MGS_GRAD_EPS).  intensity is within 1e-6
 *   absolute of a float64 evaluation for images in [0, 1].  Eight launches: one intensity, the median's six, one threshold.
 *   scratch: mgs_grad_mask_scratch_bytes(width, height) bytes (pure, monotone in both), 16-byte aligned.
 *   Needs width >= 2 and height >= 2 (reflect padding); 3 x width x height must stay below 2^31.
 *
 * mgs_frame_prepare: one preparation launch, then the eight of mgs_grad_mask on rgb_out: nine in all.
 *   colour, no maps:  rgb_out[c][y][x] = float32(double(v) / 255.0), the reference's `image / 255.0` cast to float32
 *            (dataset.py:460-465; the clamp to [0, 1] is then a no-op).
 *   colour, with maps (map_x, map_y float [H][W], source coordinates per destination pixel, dataset.py:452-453): the 8-bit
 *            pixel is first resampled as an 8-bit INTER_LINEAR remap with float maps and a constant-zero border does, in
 *            integers: sx = round-half-even(32 map_x), ix = sx >> 5 (arithmetic: -0.5 gives -1), ax = sx & 31, likewise y;
 *            weights (32-ax)(32-ay)32, ax(32-ay)32, (32-ax)ay 32, ax ay 32 (sum 2^15) on the taps (iy,ix), (iy,ix+1), (iy+1,ix),
 *            (iy+1,ix+1); a tap outside the image contributes 0; out = (sum + 2^14) >> 15 per channel.  Bit-exact against an
 *            integer restatement.  No map value whatsoever -- huge, infinite, NaN -- makes the kernel read outside the
 *            source image: such pixels are 0.  cv2 is not available to this project: parity with cv2.remap is UNPINNED.
 *   depth:   depth_out = float32(double(v) / depth_scale) (dataset.py:431,468).  Depth and segmentation are NOT remapped:
 *            the reference undistorts the colour image only.
 *   mask:    mask_out (uint8 [H,W]) = 1, except 0 where segmentation is given and bit `id` of masked_ids is set
 *            (dataset.py:445-449).  Without segmentation the mask is all ones (the reference leaves `mask` unbound there).
 *   16-byte accesses when every base given is 16-byte aligned and width is a multiple of 4, a scalar route otherwise (the
 *   gradient-mask launches choose by rgb_out, grad_mask_out and intensity_out alone).
 *   Refused with 1 and a message before anything is launched: a NULL required pointer (rgb_u8, rgb_out, mask_out,
 *   grad_mask_out, scratch), only one of the two maps, depth_u16 without depth_out or the reverse, depth given with
 *   depth_scale <= 0 or not finite, width or height < 2. */
#define MGS_EDGE_THRESHOLD 1.1f
#define MGS_GRAD_EPS 0.01f
typedef struct MgsFramePrepare {
    int32_t width, height;
    const uint8_t* rgb_u8;        /* [H][W][3] */
    const float* map_x;           /* [H][W] or NULL */
    const float* map_y;           /* [H][W] or NULL: both or neither */
    const uint16_t* depth_u16;    /* [H][W] or NULL */
    double depth_scale;           /* read when depth_u16 is given */
    const uint8_t* segmentation;  /* [H][W] ids or NULL */
    uint32_t masked_ids[8];       /* bit (id & 31) of word (id >> 5) set: id is masked out */
    float* rgb_out;               /* [3][H][W] */
    float* depth_out;             /* [H][W], given exactly when depth_u16 is */
    uint8_t* mask_out;            /* [H][W] */
    uint8_t* grad_mask_out;       /* [H][W] */
    float* intensity_out;         /* [H][W] or NULL */
    float edge_threshold, eps;    /* MGS_EDGE_THRESHOLD, MGS_GRAD_EPS */
    void* scratch;                /* mgs_grad_mask_scratch_bytes(width, height) bytes, 16-byte aligned */
} MgsFramePrepare;
size_t mgs_grad_mask_scratch_bytes(int32_t width, int32_t height);
int mgs_grad_mask(int32_t width, int32_t height, const float* rgb /* [3,H,W] */, float edge_threshold, float eps,
                  void* scratch, uint8_t* grad_mask_out /* [H,W] */, float* intensity_out /* [H,W] or NULL */, void* stream);
int mgs_frame_prepare(const MgsFramePrepare* params, void* stream);

/* ---- Stereo depth: semi-global matching of a rectified grey pair (ABI v18) --------------------------------------
 * What StereoDataset.__getitem__ (/root/reference/utils/dataset.py:595-629) does per frame -- rectify both grey images, run
 * StereoSGBM (64 disparities, block 20, uniqueness 40), turn the disparity into metric depth with a fixed baseline x fx -- as
 * twelve stream-ordered launches: no host synchronisation, no state between calls, nothing assumed about the contents of
 * scratch or outputs on entry, no atomics, every loop bounded by a launch parameter, no workgroup waits for another;
 * capturable in a hipGraph as a linear chain of kernel nodes.
 *
 * cv2 is not available to this project: the steps below are written from OpenCV's documented behaviour (mode MODE_SGBM,
 * minDisparity 0, no speckle filter) and ARE the specification; parity with cv2.StereoSGBM / cv2.remap is UNPINNED.  All
 * arithmetic up to disp16 is integer; the kernels are bit-exact against an integer restatement (tests/stereo_mirror.py).
 *
 *   L, R: uint8 [H][W].  D = num_disparities in {16, 32, 48, 64}.  Valid columns x in [D, W); W1 = W - D >= 1; H >= 1.
 *   Defaulting: block_size <= 0 -> 5; s = block_size / 2, window (2s+1)^2; p1 <= 0 -> 2; p2 <= 0 -> 5, then p2 = max(p2, p1+1);
 *            uniqueness_ratio < 0 -> 10; disp12_max_diff <= 0 -> 1; ftzero = max(pre_filter_cap, 15) | 1.
 *   0 rectify (all four maps given; otherwise the images are taken as they are): the 8-bit INTER_LINEAR remap of
 *            mgs_frame_prepare -- 1/32-pixel coordinates, weights summing to 2^15, constant-zero border, no map value reads
 *            outside the source -- on the single grey channel, with per-image float maps [H][W].
 *            rgb_out[c][y][x] = float32(double(g) / 255.0), g the rectified LEFT grey value, c = 0, 1, 2 (dataset.py:614-620).
 *   1 pre-filter, per image: g = (I[y-1][x+1] - I[y-1][x-1]) + 2 (I[y][x+1] - I[y][x-1]) + (I[y+1][x+1] - I[y+1][x-1]), rows
 *            clamped to the image; P[y][x] = clip(g, -ftzero, ftzero) + ftzero; P[y][0] = P[y][W-1] = ftzero.
 *   2 pixel cost (Birchfield-Tomasi), for J in {P, I}, x in [D, W), d in [0, D), xr = x - d: u = Jl[x], ul = (u + Jl[x-1]) / 2,
 *            ur = (u + Jl[x+1]) / 2 (integer, x +- 1 clamped to the row), u0 = min(ul, ur, u), u1 = max(ul, ur, u); v, v0, v1
 *            the same of Jr at xr; c0 = max(0, u - v1, v0 - u), c1 = max(0, v - u1, u0 - v), cost_J = min(c0, c1).
 *            pc = cost_P + cost_I <= 2 ftzero + 255.
 *   3 window: C(y,x,d) = sum over dy, dx in [-s, s] of pc(clamp(y+dy, 0, H-1), clamp(x+dx, D, W-1), d)
 *            <= (2s+1)^2 (2 ftzero + 255): 125 685 at the reference's settings, which does NOT fit 16 bits (OpenCV's short
 *            would wrap; this does not: row sums are uint16, C is uint32).
 *   4 paths, five directions r (from the left, up-left, above, up-right, the right), q = p - r, m = min_k L_r(q,k):
 *            L_r(p,d) = C(p,d) + min(L_r(q,d), L_r(q,d-1) + P1, L_r(q,d+1) + P1, m + P2) - m, L_r(q,-1) = L_r(q,D) = +inf;
 *            a predecessor outside [D,W) x [0,H) has L_r(q,.) = 0 (a path starts with L = C).  S = sum_r L_r <= 5 (C + P2).
 *   5 winner, per row, x from W-1 down to D: best = the lowest d minimising S(y,x,.), minS that minimum; the pixel is invalid
 *            if some d has S(d) (100 - uniqueness_ratio) < minS 100 and |best - d| > 1.  Passing pixels update the right-view
 *            table at x2 = x - best: if cost2[x2] > minS then cost2[x2] = minS, disp2[x2] = best (initially +inf, -1: among
 *            equal costs the largest x wins).  If 0 < best < D-1: den = max(S(best-1) + S(best+1) - 2 S(best), 1),
 *            d16 = 16 best + ((S(best-1) - S(best+1)) 16 + den) / (2 den), truncating toward zero; otherwise d16 = 16 best.
 *            Invalid pixels and every column x < D get d16 = -16.
 *   6 left-right check, after the whole row's step 5, for a valid d16: a = d16 >> 4, b = (d16 + 15) >> 4; the pixel becomes
 *            -16 if both disp2[x-a] >= 0 and |disp2[x-a] - a| > disp12_max_diff, and the same of b; an index outside
 *            [0, W) counts as disp2 < 0.
 *   7 disp16_out (int16 [H][W]) = the 3x3 median of that image, replicate border, -16 taking part as a number.
 *   8 depth_out (float [H][W]): disp = double(disp16) / 16.0; 0 -> 1e10; depth = bf / disp in double; < 0 -> 0; float32
 *            (dataset.py:608-613; the reference's bf is MGS_EUROC_BF).
 *
 * Bounds: block_size <= 63 (2s+1 <= 63, so a row sum <= 63 x 509 fits uint16), pre_filter_cap <= 127 (P is 8-bit), p1, p2 <=
 * 2^20, uniqueness_ratio <= 100; then C <= 2 020 221, S < 2^24, and S x 100 and (S << 6 | d) fit 32 bits.
 * (W - D) x H x D must stay below 2^31.
 * Launches: prepare, pre-filter, row sums, column sums, five paths, winner, table, finish = 12.
 * scratch: mgs_stereo_scratch_bytes(width, height, num_disparities) bytes (pure, monotone in each argument; 256 for sizes
 * the entry point refuses), 16-byte aligned: 178 944 256 bytes at 752 x 480 x 64 (two uint32 volumes of 84.5 MB).
 * Optional outputs: left_rect_out / right_rect_out (uint8 [H][W], the images after step 0); sum_out (int32 [H][W-D][D], the S
 * volume, for tests; NULL in the product).
 * Refused with 1 and a message before anything is launched: NULL params or a NULL required pointer (left_u8, right_u8,
 * rgb_out, disp16_out, depth_out, scratch), some but not all of the four maps, num_disparities not one of 16, 32, 48, 64,
 * width <= num_disparities, height < 1, a parameter beyond the bounds above, a bf that is not finite, a misaligned scratch. */
#define MGS_EUROC_BF 47.90639384423901
typedef struct MgsStereo {
    int32_t width, height, num_disparities;
    int32_t block_size, p1, p2, uniqueness_ratio, disp12_max_diff, pre_filter_cap;
    double bf;                    /* baseline x fx */
    const uint8_t* left_u8;       /* [H][W] */
    const uint8_t* right_u8;      /* [H][W] */
    const float* map_lx;          /* [H][W] or NULL: all four maps or none */
    const float* map_ly;
    const float* map_rx;
    const float* map_ry;
    float* rgb_out;               /* [3][H][W] */
    int16_t* disp16_out;          /* [H][W] */
    float* depth_out;             /* [H][W] */
    uint8_t* left_rect_out;       /* [H][W] or NULL */
    uint8_t* right_rect_out;      /* [H][W] or NULL */
    int32_t* sum_out;             /* [H][W-D][D] or NULL */
    void* scratch;                /* mgs_stereo_scratch_bytes(...) bytes, 16-byte aligned */
} MgsStereo;
size_t mgs_stereo_scratch_bytes(int32_t width, int32_t height, int32_t num_disparities);
int mgs_stereo_depth(const MgsStereo* params, void* stream);

/* ---- TSDF fusion of depth images and indexed triangle-mesh extraction (ABI v23) ---------------------------------
 * The specification is DESIGN.md, "TSDF fusion and mesh extraction" (tests/tsdf_mirror.py restates it in float64).
 * VOLUME: a dense grid of nx x ny x nz voxels, nx ny nz < 2^31; origin = the centre of voxel (0,0,0) in world metres, voxel =
 * the edge; centre of (i,j,k) = origin + voxel (i,j,k); linear index (k ny + j) nx + i.  Planes: float32 tsdf (initially 1),
 * weight (initially 0) and, all three or none, r, g, b (initially 0).  The caller owns and initialises them.
 * mgs_tsdf_integrate fuses one frame, one launch: per voxel centre p, in float32, pc = R p + t from `viewmatrix` (the device
 * matrix of mgs_camera.viewmatrix; never read on the host); skip if pc.z <= depth_min; pixel ix = floor(fx pc.x / pc.z + cx
 * - 0.5 + 0.5), iy likewise, skip outside the image; d = depth[iy][ix]; with `opacity`: skip if a < opacity_min, else d = d / a;
 * skip unless depth_min < d <= depth_max (depth_max <= 0: no upper bound); sdf = d - pc.z, skip if sdf < -trunc; f = min(1,
 * sdf / trunc); tsdf = (tsdf W + f) / (W + 1), colour likewise from rgb[:, iy, ix] when volume and frame both have colour,
 * weight = min(W + 1, max_weight).  Planes are touched only by voxels that reach the update.  A wave owns 64 consecutive x of
 * one row and leaves early when the row segment's bounding sphere lies behind depth_min, outside the image or beyond depth_max +
 * trunc (conservative: the result is bit-identical with MGS_TSDF_NO_CULL, a test flag).  No atomics, no host
 * synchronisation, capturable in a hipGraph; bitwise reproducible.
 * EXTRACT: marching tetrahedra (six per cell around the diagonal 000 -> 111) over the cells whose 8 corners have weight >=
 * min_weight; inside = tsdf < 0.  mgs_tsdf_extract_count (5 launches) fills `scratch` (mgs_tsdf_extract_scratch_bytes(nx, ny,
 * nz) bytes, pure and monotone, 256 for sizes the entry points refuse; nothing assumed on entry) and writes counts[2] = {V, T}
 * on the device (saturating at 2^32 - 1); the caller reads them back, allocates, and calls mgs_tsdf_extract_emit (2 launches)
 * with the same volume and scratch: vertices [V,3] float32 ordered by (owner voxel index, edge bit 0..6 = +x, +y, +z, +x+y, +y+z,
 * +x+z, +x+y+z), colors [V,3] or NULL, triangles [T,3] int32 ordered by (cell index, tetrahedron, triangle), normals towards
 * positive tsdf.  No store lands beyond V vertices or T triangles.  Scans are the library's own kernels; no atomics.
 * Refused with 1 and a message before any launch: NULL volume / frame / required plane or pointer, r, g, b not all-or-none,
 * non-positive dimensions or image size, nx ny nz >= 2^31, voxel <= 0, trunc <= 0, max_weight < 1, fx or fy <= 0, V or T >= 2^31. */
#define MGS_TSDF_NO_CULL 1
typedef struct mgs_tsdf_volume {
    int32_t nx, ny, nz;
    float origin[3];
    float voxel;
    float* tsdf;                  /* [nz][ny][nx] */
    float* weight;
    float* r;                     /* all three or none */
    float* g;
    float* b;
} mgs_tsdf_volume;
typedef struct mgs_tsdf_frame {
    int32_t width, height;
    const float* depth;           /* [H][W] */
    const float* opacity;         /* [H][W] or NULL */
    const float* rgb;             /* [3][H][W] or NULL */
    const float* viewmatrix;      /* device, 16 floats, transposed world->camera */
    float fx, fy, cx, cy;
    float trunc, depth_min, depth_max, opacity_min, max_weight;
    int32_t flags;                /* 0, or MGS_TSDF_NO_CULL */
} mgs_tsdf_frame;
int mgs_tsdf_integrate(const mgs_tsdf_volume* volume, const mgs_tsdf_frame* frame, void* stream);
size_t mgs_tsdf_extract_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
int mgs_tsdf_extract_count(const mgs_tsdf_volume* volume, float min_weight, void* scratch, uint32_t* counts /* [2] device */,
                           void* stream);
int mgs_tsdf_extract_emit(const mgs_tsdf_volume* volume, const void* scratch, float* vertices /* [V,3] */,
                          float* colors /* [V,3] or NULL */, int32_t* triangles /* [T,3] */, uint32_t V, uint32_t T, void* stream);

/* ---- Reconstruction evaluation against a ground-truth mesh (ABI v24) ------------------------------------------------
 * The specification is DESIGN.md, "Reconstruction evaluation" (tests/mesh_eval_mirror.py restates it in float64).  Every entry
 * point takes a stream, keeps no state between calls, uses no float atomics and no library kernels (sorts and scans are the
 * library's own) and is bitwise reproducible from call to call.
 *
 * mgs_nn_dist2: d2[q] = min over targets p of fma(dz, dz, fma(dy, dy, dx dx)), d = target - query in float32 (the pair formula of
 * mgs_dist2_knn); index[q] (or NULL) = the SMALLEST target index that attains it.  P == 0: d2 = +inf, index = -1; Q == 0: nothing
 * is done.  Two paths, bit-identical in both outputs: below mgs_nn_grid_min() (6144) targets an LDS-tiled all-pairs sweep,
 * from there on boxes of 64 along the Morton curve of the joint bounding box (mgs_dist2_knn's index, built for both sets; one
 * wave answers 64 neighbouring queries and prunes boxes wave-uniformly); flags force one of them for THIS call.  `scratch`:
 * mgs_nn_scratch_bytes(Q, P) bytes (pure; sized for either path; may be NULL on the all-pairs path).
 *
 * mgs_mesh_sample: N points on the triangles with keep[t] != 0 (keep NULL: all), area-weighted and stratified.  Area of a
 * triangle in float32, 0.5 |(b - a) x (c - a)|, quantised to uint64 by a power of two chosen from the vertices' bounding box
 * so that the sum of T areas stays below 2^60; inclusive integer scan (exact: the chosen triangle does not depend on scan order).
 * Sample s draws r0, r1, r2 in [0, 1) (24 bits each) from the counter hash mix(mix(seed ^ 0x9E3779B9) + 3 s + k), takes the
 * first triangle whose inclusive sum exceeds floor((s + r0) / N * total) (float64), and lies at a + sqrt(r1) (1 - r2) (b - a) +
 * sqrt(r1) r2 (c - a).  Zero-area and masked triangles are never chosen.  tri_index [N] or NULL; *area (device double, or NULL)
 * = the kept area.  A vertex index outside [0, V) is an argument error found on the device: bit 0 of *status (device word, zeroed
 * by the caller) is raised, the triangle counts as area 0 and nothing is read through it.  With no kept area the points are 0
 * and tri_index -1 (the caller reads *area).  `scratch`: mgs_mesh_sample_scratch_bytes(T) bytes.
 *
 * mgs_mesh_mark_seen: one launch per view, one lane per vertex; seen[v] (bytes, zeroed by the caller before the first view) is set
 * to 1 when pc = R p + t (`viewmatrix`: the device matrix of mgs_camera.viewmatrix) has max(depth_min, 0+) <= pc.z <= depth_max
 * (depth_max <= 0: no upper bound), its pixel -- exactly the projection and pixel rule of mgs_tsdf_integrate -- lies inside the image
 * and, with `depth` ([H][W] or NULL), depth > 0 there and pc.z <= depth + occlusion_eps.  A lane stores only its own byte.
 *
 * mgs_recon_metrics: out[0] = sum of sqrt(d2) over the finite entries (float64), out[1] = their number, out[2 + k] = how many have
 * sqrt(d2) < thresholds[k] (host array, K <= MGS_RECON_MAX_THRESHOLDS, compared in float64); all as doubles, the counts exact.
 * Per-block partial sums in a fixed order and one finishing block.  `scratch`: mgs_recon_metrics_scratch_bytes() bytes.
 * Refused with 1 and a message before any launch: negative sizes, sizes beyond 2^30, NULL required pointers, unknown or
 * contradictory flags, a mesh without vertices or triangles, non-positive image size or focal lengths, K out of range. */
#define MGS_NN_FORCE_ALL_PAIRS 1
#define MGS_NN_FORCE_MORTON 2
#define MGS_RECON_MAX_THRESHOLDS 8
int32_t mgs_nn_grid_min(void);
size_t mgs_nn_scratch_bytes(int32_t Q, int32_t P);
int mgs_nn_dist2(int32_t Q, int32_t P, const float* queries /* [Q,3] */, const float* targets /* [P,3] */, int32_t flags,
                 float* d2 /* [Q] */, int32_t* index /* [Q] or NULL */, void* scratch, void* stream);
size_t mgs_mesh_sample_scratch_bytes(int32_t T);
int mgs_mesh_sample(int32_t V, int32_t T, const float* vertices /* [V,3] */, const int32_t* triangles /* [T,3] */,
                    const uint8_t* keep /* [T] or NULL */, int32_t N, uint32_t seed, float* points /* [N,3] */,
                    int32_t* tri_index /* [N] or NULL */, double* area /* device, or NULL */, uint32_t* status /* device */,
                    void* scratch, void* stream);
int mgs_mesh_mark_seen(int32_t V, const float* vertices /* [V,3] */, const float* viewmatrix /* device, 16 floats */, int32_t W,
                       int32_t H, float fx, float fy, float cx, float cy, const float* depth /* [H][W] or NULL */, float depth_min,
                       float depth_max, float occlusion_eps, uint8_t* seen /* [V] */, void* stream);
size_t mgs_recon_metrics_scratch_bytes(void);
int mgs_recon_metrics(int32_t Q, const float* d2 /* [Q] */, int32_t K, const float* thresholds /* host [K] */,
                      double* out /* device [2 + K] */, void* scratch, void* stream);

/* ---- Triangle-mesh rendering and the Depth L1 metric (ABI v25) ---------------------------------------------------------
 * The specification is DESIGN.md, "Mesh rendering" (tests/mesh_render_mirror.py restates it in float64).
 * mgs_mesh_render: an indexed triangle mesh seen by a pinhole camera.  A world vertex goes to camera space with `viewmatrix` (the
 * device matrix of mgs_camera.viewmatrix; never read on the host); pixel (px, py) looks along d = ((px + 0.5 - cx) / fx,
 * (py + 0.5 - cy) / fy, 1).  For camera-space vertices v0, v1, v2: w0 = d . (v1 x v2), w1 = d . (v2 x v0), w2 = d . (v0 x v1),
 * S = w0 + w1 + w2; the ray hits iff S != 0 and all w >= 0 or all w <= 0 (with MGS_MESH_ONE_SIDED: only S < 0); z = (w0 z0 + w1 z1
 * + w2 z2) / S, accepted iff z >= near (a near <= 0 counts as the smallest positive float) and (far <= 0 or z <= far).  Projective:
 * no clipping.  An edge's cross product is formed from its endpoints in ascending vertex-index order and then given the sign of
 * the direction of travel, so triangles that share an edge by index leave no gap.  Per pixel the accepted hit with the smallest
 * float32 z wins, on equal bits the smallest triangle index (the minimum of bits(z) << 32 | triangle: independent of the order of
 * execution and of the triangles, bitwise reproducible).  Outputs: depth [H][W] (0: no hit), tri_id [H][W] (-1), rgb [3][H][W]
 * (sum wi ci / S of the vertex colours; bg), label [H][W] (face_labels[tri_id]; -1); each but depth may be NULL.  A triangle that
 * names a vertex outside [0, V) is skipped before any vertex is loaded and raises bit 0 of *status (device word, zeroed by the
 * caller).  Six launches (T == 0: two, the empty image), no host synchronisation, capturable in a hipGraph.  `scratch`:
 * mgs_mesh_render_scratch_bytes(T, W, H) bytes, a pure function (256 for sizes the entry point refuses).
 * mgs_depth_l1: row[0] = sum of |a - b| over the pixels where both images are > 0 (and, with max_depth > 0, both <= max_depth),
 * row[1] = their number, row[2] = the number of pixels with b > 0; device doubles, sums in a fixed order, counts exact.
 * `scratch`: mgs_depth_l1_scratch_bytes() bytes.
 * Refused with 1 and a message before any launch: negative sizes, V or T beyond 2^30, an image size of zero or above
 * MGS_MESH_RENDER_MAX_IMAGE, non-positive fx or fy, a NULL required pointer, rgb wanted without colors, label wanted without
 * face_labels, unknown flags. */
#define MGS_MESH_ONE_SIDED 1
#define MGS_MESH_NO_SMALL 2       /* test flag: no triangle is rasterised by the setup kernel (the image is bit-identical) */
#define MGS_MESH_RENDER_MAX_IMAGE 16384
typedef struct mgs_mesh_render_params {
    int32_t V, T;
    const float* vertices;        /* [V,3] world */
    const int32_t* triangles;     /* [T,3] */
    const float* colors;          /* [V,3] or NULL */
    const int32_t* face_labels;   /* [T] or NULL */
    const float* viewmatrix;      /* device, 16 floats, transposed world->camera */
    int32_t W, H;
    float fx, fy, cx, cy;
    float near, far;
    int32_t flags;                /* 0, or MGS_MESH_ONE_SIDED | MGS_MESH_NO_SMALL */
    float bg[3];
    float* depth;                 /* [H][W] */
    int32_t* tri_id;              /* [H][W] or NULL */
    float* rgb;                   /* [3][H][W] or NULL */
    int32_t* label;               /* [H][W] or NULL */
    uint32_t* status;             /* device word */
} MgsMeshRender;
size_t mgs_mesh_render_scratch_bytes(int32_t T, int32_t W, int32_t H);
int mgs_mesh_render(const MgsMeshRender* params, void* scratch, void* stream);
size_t mgs_depth_l1_scratch_bytes(void);
int mgs_depth_l1(int32_t W, int32_t H, const float* a /* [H][W] */, const float* b /* [H][W] */, float max_depth,
                 double* row /* device [3] */, void* scratch, void* stream);

/* ---- Rigid object motion: per-object SE(3) poses on the object layer (ABI v26) ---------------------------------------------
 * The specification is DESIGN.md, "Object motion" (tests/object_motion_mirror.py restates it in float64).
 * `labels` [P]: the object id of every Gaussian; `slot_of_label`: a DEVICE table of 256 int32, the pose slot 0..M-1 of an id or -1
 * (any value outside 0..M-1 counts as -1): that Gaussian is static.  Object m has the WORLD-frame pose (R_m, T_m).
 * mgs_object_transform_forward: for a moved Gaussian  x' = R_m x + T_m  (three fused multiply-adds per component) and
 * q' = quat(R_m) (x) q  in the (r, x, y, z) order of the map's rotations (quat(R): Shepperd's branches in float64, rounded
 * once); every other Gaussian is copied bit for bit.  M = 0 is a copy (R, T may be NULL).  `rots` and `rots_out` are both given
 * or both NULL.  One launch.
 * mgs_object_transform_backward: the pose is retracted as the camera's is,  T_m <- exp([rho; theta]^) T_m  with the deltas zero
 * at evaluation, so  dL/drho_m = sum g_i,  dL/dtheta_m = sum x'_i x g_i  (+ 1/2 (w gq_v - gq_w v + v x gq_v) per Gaussian with a
 * rotation gradient gq = (gq_w, gq_v) on q' = (w, v)), written to grad_tau [M,6] as rho then theta; grad_means = R_m^T g (g for a
 * static Gaussian), grad_rots = conj(quat(R_m)) (x) gq (gq).  `rots_out`, `grad_rots_out` both given or both NULL (grad_rots then
 * must be NULL); grad_means / grad_rots may be NULL: not wanted.
 * The [M,6] sums use no float atomics and are bitwise reproducible: every workgroup of 256 threads adds its 1024 Gaussians in a
 * fixed order (a wave skips a slot none of its lanes holds) and writes one row of partials, a second launch adds the rows in a
 * fixed order.  A slot without Gaussians gets exact zeros.  Two launches (M = 0: one).  `scratch`:
 * mgs_object_motion_scratch_bytes(P, M) bytes, a pure function.
 * No host synchronisation, no allocation: capturable in a hipGraph.  Refused with 1 and a message before any launch: P < 0,
 * M outside 0..MGS_MAX_MOVING_OBJECTS, a NULL required pointer (labels, slot_of_label, means..., and R, T, grad_tau, scratch
 * when M > 0), one of a rotation pair without the other. */
#define MGS_MAX_MOVING_OBJECTS 16
size_t mgs_object_motion_scratch_bytes(int32_t P, int32_t M);
int mgs_object_transform_forward(int32_t P, int32_t M, const uint8_t* labels /* [P] */,
                                 const int32_t* slot_of_label /* device [256], -1 = static */, const float* R /* [M,3,3] row-major */,
                                 const float* T /* [M,3] */, const float* means /* [P,3] */,
                                 const float* rots /* [P,4] (r,x,y,z) or NULL */, float* means_out, float* rots_out /* or NULL */,
                                 void* stream);
int mgs_object_transform_backward(int32_t P, int32_t M, const uint8_t* labels, const int32_t* slot_of_label, const float* R,
                                  const float* means_out, const float* rots_out /* or NULL */,
                                  const float* grad_means_out /* [P,3] */, const float* grad_rots_out /* [P,4] or NULL */,
                                  float* grad_means /* [P,3] or NULL */, float* grad_rots /* [P,4] or NULL */,
                                  float* grad_tau /* [M,6]: rho then theta */, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MONOGS_RASTER_H */
