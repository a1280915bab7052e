"""What the blend forward prepares for the blend backward.

Survivor masks: the default backward (blend_backward_s_kernel) does not cull for itself, it walks the 64-bit masks the forward
wave of the same quadrant left per 64-instance step.  mgs_debug_blend_mask_stats runs the cull the backward used to run beside
those masks: no instance that cull keeps may be missing from a mask.

The gradient lines of the backward's accumulator are cleared by the workgroups of blend_forward_kernel when the forward was told
of the backward (mgs_forward_preprocess(prepare_backward = scratch)): every workgroup a contiguous share of the P lines.  Checked
through the C ABI on a scratch filled with 0xFF bytes, and by the gradients of a prepared backward against those of a backward
that clears for itself.  The default backward (blend_backward_s_kernel, unsplit and split) is also held against
blend_backward_t_kernel, which shares none of its prologue.

Bars (tests/test_gpu_parity.py::_check_grads, as in test_gpu_blend_backward_split.py): relative L2 of every gradient tensor
<= 1e-4, and elementwise |got - ref| <= 1e-3 |ref| + 1e-5 max|ref| for all but a 2e-4 fraction of the elements."""
import ctypes as C
import functools

import pytest
import torch

from monogs_amd.debug import options
from monogs_amd.synthetic import make_scene, scene_settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L2_TOL, RTOL, ATOL_OF_MAX, MAX_OUTLIER_FRAC = 1e-4, 1e-3, 1e-5, 2e-4      # test_gpu_parity._check_grads


def _hold(got, ref, what):
    assert set(got) == set(ref)
    report = {}
    for k in ref:
        x, y = got[k].double(), ref[k].double()
        scale = y.abs().max().item()
        if scale == 0:                          # (a scene with nothing in view: the gradient is zero, and so must this one be)
            assert x.abs().max().item() == 0, (what, k)
            report[k] = "zero"
            continue
        rel = ((x - y).norm() / y.norm()).item()
        bad = ((x - y).abs() > RTOL * y.abs() + ATOL_OF_MAX * scale).float().mean().item()
        report[k] = (f"{rel:.2e} <= {L2_TOL:.0e}", f"{bad:.1e} <= {MAX_OUTLIER_FRAC:.0e}")
        assert rel <= L2_TOL, (what, k, rel)
        assert bad <= MAX_OUTLIER_FRAC, (what, k, bad)
    print(what, report)


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "5k":
        return make_scene(5000, "fr3_office", seed=0)
    if name == "replica":                       # 680 rows end inside a tile
        return make_scene(60000, "replica", seed=4)
    if name == "opaque":                        # early saturation: most pixels of a quadrant finish long before its walk does
        sc = make_scene(150000, "fr3_office", seed=21, mean_radius_px=10.0)
        return sc._replace(opacities=torch.full_like(sc.opacities, 0.97))
    if name == "empty_tiles":                   # bunched in the image centre over a background
        return make_scene(60000, "fr3_office", seed=5, spread=0.45, bg=(0.3, 0.6, 0.9))
    if name == "big_splats":                    # tiles of more than 1 024 instances (test_gpu_blend_backward_split.py)
        return make_scene(12000, "fr3_office", seed=4, mean_radius_px=80.0)
    raise KeyError(name)


SCENES = ("5k", "replica", "opaque", "empty_tiles", "big_splats")


# ---- gradients: the default backward against the transposed kernel ------------------------------------------------------------

def _grads(sc, pose_only):
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    scales = sc.scales if sc.scales.shape[1] == 3 else sc.scales.repeat(1, 3)
    inp = dict(means3D=sc.means3D, opacities=sc.opacities, colors_precomp=sc.colors, scales=scales, rotations=sc.rotations)
    leaves = {k: (v.to(DEV).clone() if pose_only else v.to(DEV).clone().requires_grad_(True)) for k, v in inp.items()}
    theta = torch.zeros(3, device=DEV, requires_grad=True)
    rho = torch.zeros(3, device=DEV, requires_grad=True)
    m2 = torch.zeros_like(leaves["means3D"], requires_grad=not pose_only)
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)
    out = GaussianRasterizer(st)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"],
                                 colors_precomp=leaves["colors_precomp"], scales=leaves["scales"],
                                 rotations=leaves["rotations"], theta=theta, rho=rho)
    images = [o.detach().clone() for o in (out[0], out[2], out[3])]
    ((out[0] * sc.grad_color.to(DEV)).sum() + (out[2] * sc.grad_depth.to(DEV)).sum()).backward()
    g = dict(theta=theta.grad.clone(), rho=rho.grad.clone())
    if not pose_only:
        g.update({k: v.grad.clone() for k, v in leaves.items()}, means2D=m2.grad.clone())
    return images, g


@pytest.mark.parametrize("pose_only", [False, True])
@pytest.mark.parametrize("scanned", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_default_backward_matches_the_transposed_kernel(native_lib, name, scanned, pose_only):
    """blend_bwd_split 0 and 1 cover the unsplit walk, the back walk and the front walk of blend_backward_s_kernel; the
    reference is blend_backward_t_kernel (blend_bwd_transposed = 1).  Both binning paths (radix_scanned).  The forward's
    images are those of a run whose per-tile depth sort is a launch of its own, bit for bit."""
    lib, sc = native_lib, _scene(name)
    with options(radix_scanned=scanned):
        with options(blend_bwd_transposed=1):
            img_ref, ref = _grads(sc, pose_only)
        with options(tile_sort_fused=0):
            img_unfused, _ = _grads(sc, pose_only)
        for split in (0, 1):
            with options(blend_bwd_split=split):
                img, got = _grads(sc, pose_only)
                assert lib.mgs_debug_last_backward_split() == split
            for a, b, c in zip(img, img_ref, img_unfused):
                assert torch.equal(a, b) and torch.equal(a, c)
            _hold(got, ref, f"{name} scanned={scanned} pose_only={pose_only} [split {split}]")


# ---- the forward's masks cover the backward's cull ----------------------------------------------------------------------------

@pytest.mark.parametrize("scanned", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_the_forward_masks_cover_the_backward_cull(native_lib, name, scanned):
    lib = native_lib
    with options(radix_scanned=scanned):
        a = _abi(_scene(name))
        a.render(a.preprocess(prepare=False))
        stats = torch.zeros(4, dtype=torch.int64, device=DEV)
        from monogs_amd import _lib
        from monogs_amd.rasterizer import _stream
        _lib.check(lib.mgs_debug_blend_mask_stats(C.byref(a.cam), a.P, a.R, a.geom.data_ptr(), a.binning.data_ptr(),
                                                  a.img.data_ptr(), stats.data_ptr(), _stream()), "mgs_debug_blend_mask_stats")
        steps, own, fwd, missing = stats.tolist()
    print(f"{name} scanned={scanned}: steps {steps}, kept by the own cull {own}, set bits of the forward's masks {fwd} "
          f"(+{100.0 * (fwd - own) / max(own, 1):.2f} %), kept by the own cull and missing in the mask {missing}")
    assert steps > 0 and own > 0
    assert missing == 0


# ---- cleared lines, through the C ABI ------------------------------------------------------------------------------------------

def _abi(sc):
    """debug.RawForward on the scene: preprocess (+ prepare_backward), render (exact or capacity), backward."""
    from monogs_amd.debug import RawForward
    from monogs_amd.rasterizer import GaussianRasterizationSettings
    d = lambda t: t.to(DEV)  # noqa: E731
    return RawForward(scene_settings(sc, GaussianRasterizationSettings, device=DEV), d(sc.means3D), d(sc.opacities),
                      colors_precomp=d(sc.colors), scales=d(sc.scales if sc.scales.shape[1] == 3 else sc.scales.repeat(1, 3)),
                      rotations=d(sc.rotations), grad_color=d(sc.grad_color), grad_depth=d(sc.grad_depth))


def _lines(a):                                 # [P][16] words of the accumulator
    return a.table("backward.grad_acc", torch.int32).reshape(a.P, 16)


def _prepared_forward_and_backward(lib, sc, what, capacity_of=None):
    """0xFF-filled scratch -> preprocess(prepare_backward) + render: the lines of the visible Gaussians, the pose slots and the
    six output floats are zero bits.  Then the gradients of a prepared backward against those of one that clears the same
    (caller-zeroed) scratch itself.  `capacity_of`: R -> capacity of a capacity-mode render."""
    a = _abi(sc)
    a.scratch.fill_(0xFF)
    R = a.preprocess(prepare=True)
    cap = capacity_of(R) if capacity_of else None
    a.render(cap if cap is not None else R, capacity=cap is not None)
    vis = a.radii > 0
    dirty = int((_lines(a)[vis] != 0).sum())
    print(f"{what}: P {a.P}, visible {int(vis.sum())}, num_rendered {R}, capacity {cap}, status {int(a.status.item())}, "
          f"dirty words in visible lines {dirty}")
    assert dirty == 0
    for part in ("backward.tau_part", "backward.tau"):      # the pose slots and the line that holds the six output floats
        assert int((a.table(part, torch.int32) != 0).sum()) == 0
    if cap is not None and cap < R:
        assert int(a.status.item()) & 1                 # the overflow was raised
    got = a.backward(prepared=True)
    a.scratch.zero_()
    ref = a.backward(prepared=False)
    _hold(got, ref, what)
    return a, R


@pytest.mark.parametrize("scanned", [0, 1])
@pytest.mark.parametrize("intr", ["fr3_office", "replica"])
@pytest.mark.parametrize("P", [1, 100, 5000, 20001])
def test_the_forward_clears_the_gradient_lines(native_lib, P, intr, scanned):
    """P = 1 and 100: fewer lines than tiles (most workgroups have no share); 20 001: shares that do not divide P and a last
    share cut short; 640x480 and 1200x680 (tile counts 1200 and 3225); both binning paths."""
    with options(radix_scanned=scanned):
        _prepared_forward_and_backward(native_lib, make_scene(P, intr, seed=11 + P % 7), f"P {P} {intr} scanned {scanned}")


@pytest.mark.parametrize("scanned", [0, 1])
def test_capacity_mode_overflow_still_clears(native_lib, scanned):
    with options(radix_scanned=scanned):
        _prepared_forward_and_backward(native_lib, make_scene(20001, "fr3_office", seed=131), f"capacity R // 2, scanned {scanned}",
                                       capacity_of=lambda R: max(R // 2, 1))


def test_nothing_in_view(native_lib):
    """Every Gaussian behind the camera: num_rendered = 0, no binning work, and the forward still runs and clears."""
    sc = make_scene(5000, "fr3_office", seed=3)
    pc = sc.means3D @ sc.R.T + sc.t[None, :]
    pc[:, 2] = -pc[:, 2].abs() - 1.0
    sc = sc._replace(means3D=((pc - sc.t[None, :]) @ sc.R).contiguous())
    a, R = _prepared_forward_and_backward(native_lib, sc, "behind the camera")
    assert R == 0 and int((a.radii > 0).sum()) == 0
    assert int((_lines(a) != 0).sum()) == 0             # (all P lines are cleared, visible or not)


def test_an_unprepared_forward_clears_nothing(native_lib):
    """A forward without prepare_backward leaves a 0xFF-filled scratch alone -- also right after a prepared forward that used
    the same geometry scratch; and the hand-over is good for ONE render call: a second render of the same preprocess result
    does not touch the scratch again (the caller may have freed it)."""
    lib = native_lib
    a = _abi(make_scene(5000, "fr3_office", seed=0))
    a.scratch.fill_(0xFF)
    R = a.preprocess(prepare=True)
    a.render(R)
    assert int((_lines(a) != 0).sum()) == 0
    a.scratch.fill_(0xFF)
    a.render(R)                                         # the same geometry scratch, rendered again
    assert bool((a.scratch == 0xFF).all())
    R = a.preprocess(prepare=False)
    a.render(R)
    assert bool((a.scratch == 0xFF).all())
