// extern "C" entry points of libmonogs_raster.so (see include/monogs_raster.h).
#include "common.h"

#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace mgs {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- scratch layouts ----------------------------------------------------------------------
// ONE ordered description per scratch: *_layout(dimensions, f) calls f(name, member, bytes[, min_bytes]) for every
// sub-buffer in the order it lies in memory.  A sub-buffer starts where the one before it ended, rounded up to the
// scratch's ALIGN, and takes max(bytes, min_bytes).  carve(), bytes() and mgs_debug_scratch_field() all walk these, so a
// sub-buffer is added, moved or resized here and nowhere else.
template <class F> static void geometry_layout(int P, F& f) {
    const size_t n = (size_t)P;
    f("rec", &GeometryState::rec, n * REC_FLOATS * sizeof(float));
    f("depth_key", &GeometryState::depth_key, n * sizeof(uint32_t));
    // (depth_alt .. perm, contiguous, belong to the global depth sort.  On the per-tile path, which runs none, the banded tile
    //  sort keeps its band tables there -- GeometryState::carve, band_table_bytes() -- so the scratch does not grow)
    f("depth_alt", &GeometryState::depth_alt, n * sizeof(uint32_t));
    f("iota", &GeometryState::iota, n * sizeof(uint32_t));
    f("iota_alt", &GeometryState::iota_alt, n * sizeof(uint32_t));
    f("perm", &GeometryState::perm, n * sizeof(uint32_t));
    f("point_offsets", &GeometryState::point_offsets, n * sizeof(uint32_t));
    f("scan_blocks", &GeometryState::scan_blocks, ((size_t)scan_nblocks(P, SCAN_ITEMS_PRE) + 64) * sizeof(uint32_t));
    f("clamped", &GeometryState::clamped, n * 4);
    f("rect", &GeometryState::rect, n * sizeof(uint2));
    f("rect_sorted", &GeometryState::rect_sorted, n * sizeof(uint2));
    f("scan_status", &GeometryState::scan_status, (SCAN_SMALL_MAX_BLOCKS + 1) * sizeof(uint64_t));
    f("tile_hist", &GeometryState::tile_hist, 4 * 256 * sizeof(uint32_t));
    f("sort_temp", &GeometryState::sort_temp, radix_depth_temp_bytes((uint64_t)P));      // directly behind tile_hist
    f("prepare", &GeometryState::prepare, 2 * sizeof(unsigned long long));
}
template <class F> static void image_layout(int W, int H, F& f) {
    const size_t HW = (size_t)W * H, nt = (size_t)tiles_x(W) * tiles_y(H);
    f("final_T", &ImageState::final_T, HW * 4);
    f("n_contrib", &ImageState::n_contrib, HW * 4);
    f("ranges", &ImageState::ranges, nt * sizeof(uint2));
}
size_t BinningState::fwd_mask_rows(uint64_t R, int W, int H) {
    return (size_t)(R / 64) + (size_t)tiles_x(W) * tiles_y(H) + 1;
}
template <class F> static void binning_layout(uint64_t R, int W, int H, F& f) {
    const size_t r = (size_t)R * 4;                     // (R = 0 still reserves an element per buffer)
    f("keys_a", &BinningState::keys_a, r, 4);
    f("keys_b", &BinningState::keys_b, r, 4);
    f("vals_a", &BinningState::vals_a, r, 4);
    f("vals_b", &BinningState::vals_b, r, 4);
    f("sort_temp", &BinningState::sort_temp, mgs::sort_temp_bytes(R, tile_bits(W, H)));
    f("count", &BinningState::count, 2 * sizeof(uint32_t));
    f("fwd_masks", &BinningState::fwd_masks, BinningState::fwd_mask_rows(R, W, H) * 4 * sizeof(unsigned long long));   // behind everything older
}
template <class F> static void backward_layout(int P, F& f) {
    f("grad_acc", &BackwardState::grad_acc, (size_t)P * GRAD_FLOATS * sizeof(float));
    f("tau_part", &BackwardState::tau_part, (size_t)TAU_SLOTS * 16 * sizeof(float));     // right behind the accumulator
    f("tau", &BackwardState::tau, 16 * sizeof(float));
}

// hands out the pointers of a scratch whose (256-byte-aligned) base is `base`; walked from NULL it measures the scratch
template <class S> struct Carver {
    S s{};
    char* p;
    explicit Carver(const void* base) : p((char*)align_up((size_t)base, 256)) {}
    template <class T> void operator()(const char*, T* S::*member, size_t bytes, size_t min_bytes = 0) {
        s.*member = (T*)p;
        p += align_up(bytes > min_bytes ? bytes : min_bytes, S::ALIGN);
    }
    size_t bytes() const { return (size_t)p + 256; }    // (+ 256: the caller's base need not be aligned)
};
// finds one sub-buffer by name: its offset from the aligned base and its length
struct FieldFinder {
    const char* want;
    size_t p = 0, offset = 0, bytes = 0;
    bool found = false;
    template <class T, class S> void operator()(const char* name, T* S::*, size_t n, size_t min_bytes = 0) {
        if (!strcmp(name, want)) { found = true; offset = p; bytes = n; }
        p += align_up(n > min_bytes ? n : min_bytes, S::ALIGN);
    }
};

GeometryState GeometryState::carve(void* base, int P) {
    Carver<GeometryState> c(base);
    geometry_layout(P, c);
    c.s.sort_temp_bytes = radix_depth_temp_bytes((uint64_t)P);
    // the band tables of the banded tile sort, over the global depth sort's buffers: [64 words: totals][bands x blocks: counts]
    c.s.band_totals = c.s.depth_alt;
    c.s.band_live = c.s.depth_alt + 32;
    c.s.band_counts = c.s.depth_alt + 64;
    c.s.band_room = (size_t)((char*)c.s.point_offsets - (char*)c.s.depth_alt);
    c.s.end = c.p;
    return c.s;
}
ImageState ImageState::carve(void* base, int W, int H) { Carver<ImageState> c(base); image_layout(W, H, c); return c.s; }
BinningState BinningState::carve(void* base, uint64_t R, int W, int H) {
    Carver<BinningState> c(base);
    binning_layout(R, W, H, c);
    const bool in_b = radix_result_in_b(tile_bits(W, H));
    c.s.keys_sorted = in_b ? c.s.keys_b : c.s.keys_a;
    c.s.vals_sorted = in_b ? c.s.vals_b : c.s.vals_a;
    c.s.sort_temp_bytes = mgs::sort_temp_bytes(R, tile_bits(W, H));
    return c.s;
}
BackwardState BackwardState::carve(void* base, int P) { Carver<BackwardState> c(base); backward_layout(P, c); return c.s; }
size_t GeometryState::bytes(int P) { Carver<GeometryState> c(nullptr); geometry_layout(P, c); return c.bytes(); }
size_t ImageState::bytes(int W, int H) { Carver<ImageState> c(nullptr); image_layout(W, H, c); return c.bytes(); }
size_t BinningState::bytes(uint64_t R, int W, int H) { Carver<BinningState> c(nullptr); binning_layout(R, W, H, c); return c.bytes(); }
size_t BackwardState::bytes(int P) { Carver<BackwardState> c(nullptr); backward_layout(P, c); return c.bytes(); }

ForwardStates carve_forward(const void* geometry, const void* binning, const void* image, int P, uint64_t R, int W, int H) {
    return {GeometryState::carve(const_cast<void*>(geometry), P), ImageState::carve(const_cast<void*>(image), W, H),
            BinningState::carve(const_cast<void*>(binning), R, W, H)};
}

// ---- per-stage timing with HIP events on the launch stream -------------------------------
struct StageTimer {
    hipStream_t s;
    bool on;
    hipEvent_t ev[10];
    int n = 0;
    StageTimer(hipStream_t s_, bool on_) : s(s_), on(on_) {
        if (on) for (auto& e : ev) (void)hipEventCreate(&e);
    }
    ~StageTimer() {
        if (on) for (auto& e : ev) (void)hipEventDestroy(e);
    }
    void mark() {
        if (on && n < 10) (void)hipEventRecord(ev[n++], s);
    }
    float ms(int i) {   // time between mark i and mark i+1
        float t = 0.f;
        if (on && i + 1 < n) (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]);
        return t;
    }
    void sync() {
        if (on && n) (void)hipEventSynchronize(ev[n - 1]);
    }
};

// the checks every entry point that takes a camera and a map makes first (common.h); `who`: the text's prefix, or NULL
static void entry_error(const char* who, const char* text) {
    if (who) set_error("%s: %s", who, text);
    else set_error("%s", text);
}

int check_cam(const mgs_camera* cam, const char* who) {
    if (!cam) { entry_error(who, "camera is NULL"); return 1; }
    if (cam->image_width <= 0 || cam->image_height <= 0) { entry_error(who, "image size must be positive"); return 1; }
    if (!cam->bg || !cam->viewmatrix || !cam->projmatrix || !cam->projmatrix_raw || !cam->campos) {
        entry_error(who, "camera tensors (bg, viewmatrix, projmatrix, projmatrix_raw, campos) must be non-NULL");
        return 1;
    }
    return 0;
}

// mgs_debug_set_blend_events: recorded around the blend forward / backward launch of every call while set
static hipEvent_t g_dbg_fwd_events[2] = {nullptr, nullptr}, g_dbg_bwd_events[2] = {nullptr, nullptr};

// the blend backward forms `index * 64 + slot` in 32 bits (blend.hip, bt_flush): refuse maps it cannot address
int check_map_size(int32_t P, const char* who) {
    if (P > MGS_MAX_GAUSSIANS) {
        entry_error(who, "P exceeds MGS_MAX_GAUSSIANS (2^26 - 1): the gradient-line offset of the blend backward is 32-bit");
        return 1;
    }
    return 0;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

int mgs_abi_version(void) { return MGS_ABI_VERSION; }
int mgs_binning_path(int32_t P, int32_t W, int32_t H) { return forward_plan(P, W, H, 0).per_tile ? 1 : 0; }
const char* mgs_last_error(void) { return g_err; }

size_t mgs_geometry_bytes(int32_t P) { return GeometryState::bytes(P < 0 ? 0 : P); }
size_t mgs_image_bytes(int32_t W, int32_t H) { return ImageState::bytes(W, H); }
size_t mgs_binning_bytes(uint64_t R, int32_t W, int32_t H) { return BinningState::bytes(R, W, H); }
size_t mgs_backward_bytes(int32_t P) { return BackwardState::bytes(P < 0 ? 0 : P); }
float* mgs_backward_tau(void* backward_scratch, int32_t P) { return BackwardState::carve(backward_scratch, P < 0 ? 0 : P).tau; }

int mgs_debug_scratch_field(const char* field, int32_t P, uint64_t R, int32_t W, int32_t H, uint64_t* offset, uint64_t* bytes) {
    if (!field || !offset || !bytes) { set_error("mgs_debug_scratch_field: field, offset, bytes must be non-NULL"); return 1; }
    if (P < 0) P = 0;
    const char* name = field;
    if (!strcmp(name, "binning.point_list")) name = radix_result_in_b(tile_bits(W, H)) ? "binning.vals_b" : "binning.vals_a";
    const char* dot = strchr(name, '.');
    const size_t n = dot ? (size_t)(dot - name) : 0;
    FieldFinder f{dot ? dot + 1 : ""};
    auto scratch = [&](const char* s) { return strlen(s) == n && !strncmp(name, s, n); };
    if (scratch("geometry")) geometry_layout(P, f);
    else if (scratch("image")) image_layout(W, H, f);
    else if (scratch("binning")) binning_layout(R, W, H, f);
    else if (scratch("backward")) backward_layout(P, f);
    if (!f.found) { set_error("mgs_debug_scratch_field: unknown field \"%s\"", field); return 1; }
    *offset = f.offset;
    *bytes = f.bytes;
    return 0;
}

int mgs_forward_preprocess(const mgs_camera* cam, int32_t P, const float* means3D, const float* shs,
                           const float* colors_precomp, const float* opacities, const float* scales,
                           const float* rotations, const float* cov3D_precomp, void* geometry, int32_t* radii,
                           void* prepare_backward, uint64_t* num_rendered, const uint32_t* prev_status,
                           uint32_t* prev_status_out, mgs_timing* timing, void* stream) {
    if (check_cam(cam)) return 1;
    if (P < 0) { set_error("P must be >= 0"); return 1; }
    if (check_map_size(P)) return 1;
    if (num_rendered) *num_rendered = 0;        // NULL = capacity mode: no read-back, no stream sync
    if (prev_status_out) *prev_status_out = 0;
    if (P == 0) {
        if (prev_status && prev_status_out) {   // nothing to render, but the caller still wants the earlier forward's verdict
            MGS_HIP(hipMemcpyAsync(prev_status_out, prev_status, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
            MGS_HIP(hipStreamSynchronize((hipStream_t)stream));
        }
        return 0;
    }
    if (!means3D || !opacities || !geometry || !radii) { set_error("means3D, opacities, geometry, radii must be non-NULL"); return 1; }
    if ((shs == nullptr) == (colors_precomp == nullptr)) {
        set_error("Please provide excatly one of either SHs or precomputed colors!");
        return 1;
    }
    const bool have_sr = scales != nullptr || rotations != nullptr;
    if ((have_sr && (!scales || !rotations || cov3D_precomp)) || (!have_sr && !cov3D_precomp)) {
        set_error("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
        return 1;
    }
    if (shs && (cam->sh_degree < 0 || cam->sh_degree > 3 || cam->sh_coeffs < (cam->sh_degree + 1) * (cam->sh_degree + 1))) {
        set_error("sh_degree must be 0..3 and shs must hold at least (degree+1)^2 coefficients");
        return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    GeometryState g = GeometryState::carve(geometry, P);
    const ForwardPlan plan = forward_plan(P, cam->image_width, cam->image_height, cam->flags);
    StageTimer tm(s, timing != nullptr);
    tm.mark();
    if (int rc = launch_preprocess_forward(plan, *cam, means3D, shs, colors_precomp, opacities, scales, rotations,
                                           cov3D_precomp, g, radii,
                                           prepare_backward ? BackwardState::carve(prepare_backward, P).grad_acc : nullptr, s)) return rc;
    tm.mark();
    // (per-tile path: no global depth sort, the scan runs in index order -- binning.hip)
    if (!plan.per_tile)
        if (int rc = launch_depth_sort(plan, g, s)) return rc;
    tm.mark();
    if (int rc = launch_scan(plan, g, s)) return rc;
    tm.mark();
    if (num_rendered) {
        uint32_t total = 0, sort_errors[RADIX_ERROR_WORDS] = {0, 0, 0, 0};
        MGS_HIP(hipMemcpyAsync(&total, g.scan_blocks + plan.scan_blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, s));   // grand total
        MGS_HIP(hipMemcpyAsync(sort_errors, radix_depth_error_flag(g.sort_temp, (uint64_t)P), sizeof(sort_errors),
                               hipMemcpyDeviceToHost, s));
        // the status word of an EARLIER forward on this stream rides along: its kernels are done by the time this copy runs,
        // so a tile-sort timeout of the exact path is seen one forward later at no extra synchronisation
        if (prev_status && prev_status_out)
            MGS_HIP(hipMemcpyAsync(prev_status_out, prev_status, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        MGS_HIP(hipStreamSynchronize(s));
        if (sort_errors[0] | sort_errors[1] | sort_errors[2] | sort_errors[3]) { set_error("depth sort: a look-back spin timed out (results invalid)"); return 3; }
        *num_rendered = total;
    }
    if (timing) {
        if (!num_rendered) MGS_HIP(hipStreamSynchronize(s));
        timing->preprocess_ms = tm.ms(0);
        timing->depth_sort_ms = plan.per_tile ? 0.f : tm.ms(1);
        timing->scan_ms = tm.ms(2);
    }
    return 0;
}

static int forward_render_impl(const mgs_camera* cam, int32_t P, uint64_t R, bool capacity, void* geometry,
                               void* binning, void* image, float* out_color, float* out_depth, float* out_opacity,
                               int32_t* n_touched, uint32_t* overflow, mgs_timing* timing, void* stream) {
    if (check_cam(cam)) return 1;
    if (P < 0) { set_error("P must be >= 0"); return 1; }
    if (check_map_size(P)) return 1;
    if (!image || !out_color || !out_depth || !out_opacity) { set_error("image scratch and outputs must be non-NULL"); return 1; }
    if (P > 0 && (!geometry || !n_touched)) { set_error("geometry and n_touched must be non-NULL"); return 1; }
    if (R > 0 && !binning) { set_error("binning scratch is NULL"); return 1; }
    if (R >= (1ull << 32)) { set_error("num_rendered exceeds 2^32-1"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    const int W = cam->image_width, H = cam->image_height;
    // (P == 0: the plan's R is 0 whatever the caller passed; geometry may be NULL)
    const ForwardPlan plan = forward_plan(P, W, H, cam->flags).render(R, capacity);
    R = plan.R;
    auto [g, img, b] = carve_forward(geometry, binning, image, P, R, W, H);
    StageTimer tm(s, timing != nullptr);
    uint32_t* const count = (capacity && binning) ? b.count : nullptr;      // capacity mode: the live count stays on the device
    tm.mark();
    if (int rc = launch_duplicate(plan, g, b, img, n_touched, count, overflow, s)) return rc;
    tm.mark();
    if (int rc = launch_sort(plan, g, b, img, count, s)) return rc;
    const uint32_t* sort_err = R > 0 ? radix_error_flag(b.sort_temp, R, plan.tile_bits) : nullptr;
    // per-tile depth order: each tile's list, in index order now, sorted by depth in LDS -- by the blend forward's workgroup
    // of the tile (timed with the blend forward), or by a launch of its own (timed with the sort)
    const TileSortArgs ts = plan.sort_tiles ? tile_sort_args(plan, g, b, count) : TileSortArgs{};
    if (plan.sort_tiles && !plan.tile_sort_fused)
        if (int rc = launch_tile_depth_sort(plan, ts, img, sort_err, s)) return rc;
    tm.mark();
    if (g_dbg_fwd_events[0]) MGS_HIP(hipEventRecord(g_dbg_fwd_events[0], s));
    if (int rc = launch_blend_forward(plan, *cam, g, b, img, out_color, out_depth, out_opacity, n_touched, sort_err, overflow,
                                      ts, s)) return rc;
    if (g_dbg_fwd_events[1]) MGS_HIP(hipEventRecord(g_dbg_fwd_events[1], s));
    tm.mark();
    if (timing) {
        tm.sync();
        timing->duplicate_ms = tm.ms(0);
        timing->sort_ms = tm.ms(1);
        timing->ranges_ms = 0.f;              // (no ranges launch since round 4: the tile sort's final pass writes them)
        timing->blend_fwd_ms = tm.ms(2);
    }
    return 0;
}

int mgs_forward_render(const mgs_camera* cam, int32_t P, uint64_t R, void* geometry, void* binning, void* image,
                       float* out_color, float* out_depth, float* out_opacity, int32_t* n_touched,
                       uint32_t* status, mgs_timing* timing, void* stream) {
    return forward_render_impl(cam, P, R, false, geometry, binning, image, out_color, out_depth, out_opacity, n_touched,
                               status, timing, stream);
}

int mgs_forward_render_capacity(const mgs_camera* cam, int32_t P, uint64_t capacity, void* geometry, void* binning,
                                void* image, float* out_color, float* out_depth, float* out_opacity,
                                int32_t* n_touched, uint32_t* overflow, mgs_timing* timing, void* stream) {
    if (capacity == 0) { set_error("capacity must be > 0"); return 1; }
    return forward_render_impl(cam, P, capacity, true, geometry, binning, image, out_color, out_depth, out_opacity,
                               n_touched, overflow, timing, stream);
}

int mgs_forward_capacity(const mgs_camera* cam, int32_t P, const float* means3D, const float* shs,
                         const float* colors_precomp, const float* opacities, const float* scales, const float* rotations,
                         const float* cov3D_precomp, void* geometry, int32_t* radii, void* prepare_backward,
                         uint64_t capacity, void* binning, void* image, float* out_color, float* out_depth,
                         float* out_opacity, int32_t* n_touched, uint32_t* overflow, mgs_timing* timing, void* stream) {
    if (int rc = mgs_forward_preprocess(cam, P, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                        geometry, radii, prepare_backward, nullptr, nullptr, nullptr, timing, stream)) return rc;
    return mgs_forward_render_capacity(cam, P, capacity, geometry, binning, image, out_color, out_depth, out_opacity,
                                       n_touched, overflow, timing, stream);
}

int mgs_backward(const mgs_camera* cam, int32_t P, uint64_t R, const float* means3D, const float* shs,
                 const float* colors_precomp, const float* opacities, const float* scales, const float* rotations,
                 const float* cov3D_precomp, const int32_t* radii, const void* geometry, const void* binning,
                 const void* image, const float* dL_dcolor, const float* dL_ddepth, const float* out_color,
                 const float* out_depth, float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                 float* dL_dscales, float* dL_drotations, float* dL_dtau, void* backward_scratch,
                 int32_t scratch_prepared, mgs_timing* timing, void* stream) {
    if (check_cam(cam)) return 1;
    if (P < 0) { set_error("P must be >= 0"); return 1; }
    if (check_map_size(P)) return 1;
    hipStream_t s = (hipStream_t)stream;
    // MGS_FLAG_INTRINSICS_GRAD: dL_dtau is ten floats, (rho, theta, dfx, dfy, dcx, dcy)
    const bool intr = (cam->flags & MGS_FLAG_INTRINSICS_GRAD) != 0;
    if (intr && !dL_dtau) { set_error("MGS_FLAG_INTRINSICS_GRAD needs dL_dtau (ten floats)"); return 1; }
    const size_t tau_bytes = (intr ? 10 : 6) * sizeof(float);
    if (P == 0) {
        if (dL_dtau) MGS_HIP(zero_fill(dL_dtau, tau_bytes, s));
        return 0;
    }
    if (!means3D || !opacities || !radii || !geometry || !image || !dL_dcolor || !dL_ddepth || !backward_scratch) {
        set_error("means3D, opacities, radii, geometry, image, dL_dcolor, dL_ddepth, backward_scratch must be non-NULL");
        return 1;
    }
    if (R > 0 && !binning) { set_error("binning scratch is NULL"); return 1; }
    const int W = cam->image_width, H = cam->image_height;
    auto [g, img, b] = carve_forward(geometry, binning, image, P, R, W, H);
    const BackwardState bw = BackwardState::carve(backward_scratch, P);
    float* grad_acc = bw.grad_acc;
    StageTimer tm(s, timing != nullptr);
    // (the pose-gradient slots sit right behind the accumulator: one clear covers both)
    float* tau_part = (dL_dtau && (P + 255) / 256 > TAU_DIRECT_MAX_BLOCKS) ? bw.tau_part : nullptr;
    if (scratch_prepared) {
        // the matching forward cleared the lines of the visible Gaussians, the slots and the whole 16-float line of dL/dtau
        if (dL_dtau && dL_dtau != bw.tau) {
            set_error("scratch_prepared: dL_dtau must be mgs_backward_tau(backward_scratch, P)");
            return 1;
        }
    } else {
        MGS_HIP(zero_fill2(grad_acc, (size_t)P * GRAD_FLOATS * sizeof(float) + (tau_part ? (size_t)TAU_SLOTS * 16 * sizeof(float) : 0),
                           dL_dtau, tau_bytes, s));
    }
    tm.mark();
    if (R > 0) {
        // colours / opacities take no gradient and do not feed the geometry (no SH): the lighter blend backward
        const bool pose_only = !dL_dcolors && !dL_dopacity && !dL_dsh && !shs;
        if (g_dbg_bwd_events[0]) MGS_HIP(hipEventRecord(g_dbg_bwd_events[0], s));
        if (int rc = launch_blend_backward(*cam, g, b, img, dL_dcolor, dL_ddepth, out_color, out_depth, grad_acc, pose_only, R, s)) return rc;
        if (g_dbg_bwd_events[1]) MGS_HIP(hipEventRecord(g_dbg_bwd_events[1], s));
    }
    tm.mark();
    GeomBackwardArgs a;
    a.means3D = means3D; a.shs = shs; a.colors_precomp = colors_precomp; a.opacities = opacities;
    a.scales = scales; a.rotations = rotations; a.cov3D_precomp = cov3D_precomp; a.radii = radii;
    a.grad_acc = grad_acc;
    a.dL_dmeans2D = dL_dmeans2D; a.dL_dcolors = dL_dcolors; a.dL_dopacity = dL_dopacity;
    a.dL_dmeans3D = dL_dmeans3D; a.dL_dcov3D = dL_dcov3D; a.dL_dsh = dL_dsh; a.dL_dscales = dL_dscales;
    a.dL_drotations = dL_drotations; a.dL_dtau = dL_dtau; a.tau_part = tau_part;
    if (int rc = launch_geom_backward(*cam, P, g, a, s)) return rc;
    tm.mark();
    if (timing) {
        tm.sync();
        timing->blend_bwd_ms = tm.ms(0);
        timing->geom_bwd_ms = tm.ms(1);
    }
    return 0;
}

static int check_features(const mgs_camera* cam, int32_t P, int32_t K) {
    if (check_cam(cam)) return 1;
    if (P < 0) { set_error("P must be >= 0"); return 1; }
    if (check_map_size(P)) return 1;
    if (K < 1 || K > MGS_MAX_FEATURE_CHANNELS) { set_error("K must be 1..MGS_MAX_FEATURE_CHANNELS (256)"); return 1; }
    return 0;
}

int mgs_features_forward(const mgs_camera* cam, int32_t P, int32_t K, uint64_t num_rendered, const void* geometry,
                         const void* binning, const void* image, const float* features, const float* bg, float* out,
                         int32_t* labels, float min_opacity, void* stream) {
    if (check_features(cam, P, K)) return 1;
    if (!out) { set_error("out must be non-NULL"); return 1; }
    if (P > 0 && (!geometry || !image || !features)) { set_error("geometry, image, features must be non-NULL"); return 1; }
    if (P > 0 && num_rendered > 0 && !binning) { set_error("binning scratch is NULL"); return 1; }
    const int W = cam->image_width, H = cam->image_height;
    auto [g, img, b] = carve_forward(geometry, binning, image, P, num_rendered, W, H);
    return launch_features_forward(*cam, P, K, g, b, img, features, bg, out, labels, min_opacity, (hipStream_t)stream);
}

int mgs_features_backward(const mgs_camera* cam, int32_t P, int32_t K, uint64_t num_rendered, const void* geometry,
                          const void* binning, const void* image, const float* dL_dout, float* dL_dfeatures, void* stream) {
    if (check_features(cam, P, K)) return 1;
    if (P == 0) return 0;
    if (!geometry || !image || !dL_dout || !dL_dfeatures) { set_error("geometry, image, dL_dout, dL_dfeatures must be non-NULL"); return 1; }
    if (num_rendered > 0 && !binning) { set_error("binning scratch is NULL"); return 1; }
    const int W = cam->image_width, H = cam->image_height;
    auto [g, img, b] = carve_forward(geometry, binning, image, P, num_rendered, W, H);
    return launch_features_backward(*cam, P, K, g, b, img, dL_dout, dL_dfeatures, (hipStream_t)stream);
}

size_t mgs_viewer_scratch_bytes(int32_t W, int32_t H) { return (W > 0 && H > 0) ? viewer_scratch_bytes(W, H) : 0; }

int mgs_viewer_ellipsoids(const mgs_camera* cam, int32_t P, uint64_t num_rendered, const void* geometry, const void* binning,
                          const void* image, float threshold, float* out, int32_t* hit, void* stream) {
    if (check_cam(cam)) return 1;
    if (P < 0) { set_error("P must be >= 0"); return 1; }
    if (check_map_size(P)) return 1;
    if (!(threshold >= 1.0f / 255.0f && threshold < 1.0f)) { set_error("threshold must lie in [1/255, 1)"); return 1; }
    if (!out) { set_error("out must be non-NULL"); return 1; }
    if (P > 0 && (!geometry || !image)) { set_error("geometry, image must be non-NULL"); return 1; }
    if (P > 0 && num_rendered > 0 && !binning) { set_error("binning scratch is NULL"); return 1; }
    const int W = cam->image_width, H = cam->image_height;
    auto [g, img, b] = carve_forward(geometry, binning, image, P, num_rendered, W, H);
    return launch_viewer_ellipsoids(*cam, P, g, b, img, threshold, out, hit, (hipStream_t)stream);
}

int mgs_viewer_lines(int32_t W, int32_t H, const int32_t* segments, int32_t n_segments, void* scratch, void* stream) {
    if (W <= 0 || H <= 0) { set_error("image size must be positive"); return 1; }
    if (n_segments < 0 || (n_segments > 0 && !segments)) { set_error("n_segments must be >= 0 and segments non-NULL"); return 1; }
    if (!scratch || (size_t)scratch % 256 != 0) { set_error("scratch must be non-NULL and 256-byte aligned"); return 1; }
    return launch_viewer_lines(W, H, segments, n_segments, scratch, (hipStream_t)stream);
}

int mgs_viewer_compose(int32_t mode, int32_t W, int32_t H, const float* src, const uint8_t* lut, const uint8_t* seg_rgb,
                       int32_t n_segments, void* scratch, uint8_t* out, void* stream) {
    if (mode < MGS_VIEWER_RGB || mode > MGS_VIEWER_ELLIPSOIDS) { set_error("unknown viewer mode"); return 1; }
    if (W <= 0 || H <= 0) { set_error("image size must be positive"); return 1; }
    if (!src || !out) { set_error("src, out must be non-NULL"); return 1; }
    if ((mode == MGS_VIEWER_DEPTH || mode == MGS_VIEWER_TIME) && !lut) { set_error("depth and time need the colour table"); return 1; }
    if (n_segments < 0 || (n_segments > 0 && !seg_rgb)) { set_error("n_segments must be >= 0 and seg_rgb non-NULL"); return 1; }
    if ((mode == MGS_VIEWER_DEPTH || n_segments > 0) && (!scratch || (size_t)scratch % 256 != 0)) {
        set_error("scratch must be non-NULL and 256-byte aligned");
        return 1;
    }
    return launch_viewer_compose(mode, W, H, src, lut, seg_rgb, n_segments, scratch, out, (hipStream_t)stream);
}

int mgs_debug_blend_stats(const mgs_camera* cam, int32_t P, uint64_t R, const void* geometry, const void* binning,
                           const void* image, uint64_t* stats_dev, void* stream) {
    if (check_cam(cam)) return 1;
    if (!geometry || !image || !stats_dev || (R > 0 && !binning)) { set_error("bad arguments"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    MGS_HIP(zero_fill(stats_dev, MGS_BLEND_STATS_WORDS * sizeof(uint64_t), s));
    if (P == 0 || R == 0) return 0;
    const int W = cam->image_width, H = cam->image_height;
    auto [g, img, b] = carve_forward(geometry, binning, image, P, R, W, H);
    return launch_blend_backward_stats(*cam, g, b, img, (unsigned long long*)stats_dev, s);
}

int mgs_debug_blend_mask_stats(const mgs_camera* cam, int32_t P, uint64_t R, const void* geometry, const void* binning,
                               const void* image, uint64_t* stats_dev, void* stream) {
    if (check_cam(cam)) return 1;
    if (!geometry || !image || !stats_dev || (R > 0 && !binning)) { set_error("bad arguments"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    MGS_HIP(zero_fill(stats_dev, MGS_BLEND_MASK_STATS_WORDS * sizeof(uint64_t), s));
    if (P == 0 || R == 0) return 0;
    const int W = cam->image_width, H = cam->image_height;
    auto [g, img, b] = carve_forward(geometry, binning, image, P, R, W, H);
    return launch_blend_mask_stats(*cam, g, b, img, (unsigned long long*)stats_dev, s);
}

int mgs_debug_valu_ceiling(float* out, int32_t iters, void* stream) {
    if (!out || iters < 1) { set_error("mgs_debug_valu_ceiling: bad arguments"); return 1; }
    return launch_valu_ceiling(out, iters, (hipStream_t)stream);
}

int mgs_debug_last_backward_split(void) { return g_dbg_last_bwd_split; }
int mgs_debug_last_tile_sort_bands(void) { return g_dbg_last_tile_sort_bands; }

int mgs_debug_forward_plan(int32_t P, int32_t W, int32_t H, int32_t flags, uint64_t R, int32_t capacity_mode, uint64_t* out) {
    if (!out || P < 0 || W <= 0 || H <= 0 || R >= (1ull << 32)) { set_error("mgs_debug_forward_plan: out non-NULL, P >= 0, W, H > 0, R < 2^32"); return 1; }
    const ForwardPlan p = forward_plan(P, W, H, flags).render(R, capacity_mode != 0);
    auto u = [](int v) { return (uint64_t)(uint32_t)v; };
    const uint64_t words[MGS_PLAN_WORDS] = {
        u(p.P), u(p.W), u(p.H), u(p.flags), p.capacity_mode, u(p.tiles_x), u(p.tiles_y), u(p.ntiles), u(p.tile_bits), p.small_grid,
        p.per_tile, u(p.scan_items), u(p.scan_shift), u(p.scan_blocks), p.scan_small, u(p.bands_counted), p.rect_packed, p.exclusive,
        p.R, p.r_cap, p.slot_major, u(p.bands), p.count_digits, u(p.key_shift), u(p.depth_lo_bits), p.sort_tiles, p.tile_sort_fused,
        u(p.dup_threads),
        // the two scratch sizes the banded decision compares (no banded pass without counted bands)
        p.bands_counted ? radix_banded_temp_bytes(p.R, p.bands_counted) : 0, radix_temp_bytes(p.R, p.tile_bits)};
    static_assert(MGS_PLAN_TWO_PASS_BYTES == MGS_PLAN_WORDS - 1 && MGS_PLAN_PER_TILE == 10 && MGS_PLAN_R == 18, "the order of MGS_PLAN_*");
    memcpy(out, words, sizeof(words));
    return 0;
}

int mgs_debug_set_radix_spin_limit(uint32_t limit) { return set_radix_spin_limit(limit); }

int mgs_debug_set_blend_events(void* fwd_start, void* fwd_end, void* bwd_start, void* bwd_end) {
    if ((fwd_start == nullptr) != (fwd_end == nullptr) || (bwd_start == nullptr) != (bwd_end == nullptr)) {
        set_error("mgs_debug_set_blend_events: a pair is both events or neither");
        return 1;
    }
    g_dbg_fwd_events[0] = (hipEvent_t)fwd_start; g_dbg_fwd_events[1] = (hipEvent_t)fwd_end;
    g_dbg_bwd_events[0] = (hipEvent_t)bwd_start; g_dbg_bwd_events[1] = (hipEvent_t)bwd_end;
    return 0;
}

static int g_opt_debug_sort_exclusive = 0;   // mgs_debug_set_option("debug_sort_exclusive", 1): mgs_debug_sort_pairs sorts as under
                                             // MGS_FLAG_EXCLUSIVE_DEVICE (block ids as tile ids)
size_t mgs_debug_sort_temp_bytes(uint64_t n, int32_t bits) { return radix_temp_bytes(n, bits); }
int mgs_debug_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t* keys_alt, uint32_t* vals_alt, uint64_t n, int32_t bits,
                         void* temp, void* stream) {
    if (bits < 1 || bits > 32 || (n && (!keys || !vals || !keys_alt || !vals_alt || !temp))) {
        set_error("mgs_debug_sort_pairs: bad arguments");
        return 1;
    }
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    RadixSortOptions o;
    o.exclusive = g_opt_debug_sort_exclusive != 0;
    if (int rc = radix_sort_pairs(keys, vals, keys_alt, vals_alt, n, bits, temp, s, o)) return rc;
    if (radix_result_in_b(bits)) {
        MGS_HIP(hipMemcpyAsync(keys, keys_alt, n * 4, hipMemcpyDeviceToDevice, s));
        MGS_HIP(hipMemcpyAsync(vals, vals_alt, n * 4, hipMemcpyDeviceToDevice, s));
    }
    uint32_t err[RADIX_ERROR_WORDS];
    MGS_HIP(hipMemcpyAsync(err, radix_error_flag(temp, n, bits), sizeof(err), hipMemcpyDeviceToHost, s));
    MGS_HIP(hipStreamSynchronize(s));
    if (err[0] | err[1] | err[2] | err[3]) { set_error("mgs_debug_sort_pairs: a look-back spin timed out"); return 2; }
    return 0;
}

int mgs_debug_set_option(const char* name, int64_t value) {
    // name, variable, default, largest value (larger ones saturate).  Any negative value restores the default.
    static const struct { const char* name; int* var; int def, max; } options[] = {
        {"radix_scanned", &g_opt_radix_scanned, -1, INT_MAX},
        {"radix_ballot_rank", &g_opt_radix_ballot_rank, 0, 1},
        {"radix_xcd_band", &g_opt_radix_xcd_band, 1, 1},
        {"debug_sort_exclusive", &g_opt_debug_sort_exclusive, 0, 1},
        {"dup_slot_major", &g_opt_dup_slot_major, -1, 1},
        {"blend_bwd_transposed", &g_opt_blend_bwd_transposed, 2, INT_MAX},     // (2 / 1 / 0 name one kernel each)
        {"blend_bwd_split", &g_opt_blend_bwd_split, -1, INT_MAX},
        {"blend_bwd_split_min", &g_opt_blend_bwd_split_min, 4, INT_MAX},       // (both clamped where they are used: blend.hip)
        {"blend_bwd_split_frac", &g_opt_blend_bwd_split_frac, 32, INT_MAX},
        {"scan_small", &g_opt_scan_small, -1, 1},
        {"pre_scan", &g_opt_pre_scan, -1, 1},
        {"tile_sort_banded", &g_opt_tile_sort_banded, 1, 1},
        {"tile_sort_fused", &g_opt_tile_sort_fused, 1, 1},
        {"knn_grid_min", &g_opt_knn_grid_min, -1, INT_MAX},
    };
    for (const auto& o : options) {
        if (!name || strcmp(name, o.name)) continue;
        *o.var = value < 0 ? o.def : value > o.max ? o.max : (int)value;
        // the one row with a side effect: 2 SET BY HAND is the unsplit s-kernel, the A/B partner of 1 and 0
        if (o.var == &g_opt_blend_bwd_transposed) g_opt_blend_bwd_transposed_set = value >= 0;
        return 0;
    }
    set_error("mgs_debug_set_option: unknown option");
    return 1;
}

int mgs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* visible, void* stream) {
    (void)projmatrix;
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !visible))) { set_error("bad arguments"); return 1; }
    return launch_mark_visible(P, means3D, viewmatrix, visible, (hipStream_t)stream);
}

size_t mgs_knn_scratch_bytes(int32_t P) { return knn_scratch_bytes(P); }

int mgs_dist2_knn(int32_t P, const float* points, float* out, void* scratch, void* stream) {
    if (P < 0 || (P > 0 && (!points || !out))) { set_error("bad arguments"); return 1; }
    return launch_knn(P, points, out, scratch, (hipStream_t)stream);
}

}  // extern "C"
