"""Intrinsics gradient, what can be checked without a GPU: the ABI constants, ``Intrinsics.set``, the fixtures of
tests/test_gpu_intrinsics.py (their finite-difference reference must not sit on a threshold) and the compiler's resource report of
the per-Gaussian backward with and without the intrinsics variant."""
import os
import re

import pytest
import torch

import intrinsics_scenes as S
from monogs_amd import _lib
from monogs_amd.frames import Intrinsics
from resource_report import resource_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "monogs_raster.h")) as f:
        return f.read()


def test_abi_version_and_flag(native_lib):
    text = _header()
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 28
    assert native_lib.mgs_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define MGS_FLAG_INTRINSICS_GRAD (\d+)", text).group(1)) == _lib.FLAG_INTRINSICS_GRAD == 2
    assert int(re.search(r"#define MGS_FLAG_EXCLUSIVE_DEVICE (\d+)", text).group(1)) == _lib.FLAG_EXCLUSIVE_DEVICE == 1


def test_intrinsics_set_equals_a_fresh_object():
    k0 = dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6, W=640, H=480)
    new = dict(k0, fx=548.25, fy=530.5, cx=322.75, cy=245.125)
    intr = Intrinsics(k0, "cpu", learnable=True)
    old_matrix = intr.projection_matrix
    assert isinstance(intr.delta, torch.nn.Parameter) and intr.delta.shape == (4,) and intr.delta.abs().max().item() == 0
    assert not hasattr(Intrinsics(k0, "cpu"), "delta")
    intr.set(new["fx"], new["fy"], new["cx"], new["cy"])
    fresh = Intrinsics(new, "cpu")
    assert intr.projection_matrix is not old_matrix                     # every cached_camera_tensors entry misses
    assert torch.equal(intr.projection_matrix, fresh.projection_matrix)
    assert not torch.equal(intr.projection_matrix, old_matrix)
    assert (intr.fx, intr.fy, intr.cx, intr.cy) == (fresh.fx, fresh.fy, fresh.cx, fresh.cy)
    assert (intr.FoVx, intr.FoVy) == (fresh.FoVx, fresh.FoVy) and intr.k == fresh.k
    assert (intr.height, intr.width) == (fresh.height, fresh.width)
    assert intr.delta.abs().max().item() == 0


@pytest.mark.parametrize("name", list(S.SCENES))
def test_fixture_reference_is_off_every_threshold(name):
    """Central differences of the float64 oracle at step h and h / 2 agree to 1e-6 relative in each of fx, fy, cx, cy (tanfov,
    projmatrix_raw and projmatrix rebuilt at every step): no decision flips inside the stencil for the seeds fixed in
    intrinsics_scenes.py, and the reference of the GPU test is a derivative."""
    a, b = S.central_differences(name, S.H_FD), S.central_differences(name, S.H_FD / 2)
    assert a.abs().min().item() > 0, a
    rel = ((a - b).abs() / a.abs()).max().item()
    print(f"{name}: d/d(fx, fy, cx, cy) = {a.tolist()}, h vs h/2 worst relative difference {rel:.2e}")
    assert rel <= 1e-6, (a, b)


def test_clamped_fixture_holds_clamped_gaussians_that_reach_the_image():
    cx, cy, seen = S.clamp_flags("clamped")
    assert (cx & seen).sum().item() >= 8 and (cy & seen).sum().item() >= 8, ((cx & seen).sum(), (cy & seen).sum())


def test_slots_fixture_takes_the_slot_path():
    sc, inp, _ = S.fixture("slots70001")
    assert inp["means3D"].shape[0] > 256 * 256                           # workgroups of 256 > TAU_DIRECT_MAX_BLOCKS (csrc/common.h)


# geom_backward_kernel<SH, COV> of the parent commit 16826a4 ("Per-tile binning: band instances at emission, one tile-sort
# pass"), from a build of that commit: (VGPRs, LDS bytes per block, scratch bytes per lane)
PARENT = {(False, True): (69, 20576, 0), (False, False): (96, 20576, 0), (True, True): (96, 20576, 0), (True, False): (97, 20576, 0)}


def _geom(kernels, sh, cov, intr):
    b = lambda v: f"Lb{int(v)}E"  # noqa: E731
    (name,) = [n for n in kernels if "geom_backward_kernel" in n and f"I{b(sh)}{b(cov)}{b(intr)}E" in n]
    r = kernels[name]
    return int(r["VGPRs"]), int(r["LDS Size [bytes/block]"]), int(r["ScratchSize [bytes/lane]"])


def test_existing_instantiations_keep_their_resources_and_the_variant_does_not_spill(tmp_path):
    kernels = resource_report("preprocess.hip", tmp_path)[0]
    for (sh, cov), want in PARENT.items():
        assert _geom(kernels, sh, cov, False) == want, (sh, cov)
        vgprs, lds, scratch = _geom(kernels, sh, cov, True)
        print(f"geom_backward_kernel<{sh}, {cov}, true>: {vgprs} VGPRs, {lds} B LDS, {scratch} B scratch (default: {want})")
        assert scratch == 0, (sh, cov)

