"""The `fused_ssim` drop-in without a GPU: the module-name contract and the reference's call sites
(tests/golden/ssim_seam.json, written by tests/golden/make_golden_ssim.py), the C ABI's argument errors, the Python argument
errors, and the float64 checker of the GPU tests (tests/ssim_oracle.py) pinned by an independent scipy evaluation."""
import inspect
import json
import os
import re

import pytest
import torch

import ssim_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEAM = json.load(open(os.path.join(ROOT, "tests", "golden", "ssim_seam.json")))
NEW_SYMBOLS = ("mgs_ssim_scratch_bytes", "mgs_ssim_forward", "mgs_ssim_backward", "mgs_refine_loss_forward",
               "mgs_refine_loss_backward", "mgs_refine_loss_grads")


def test_module_name_contract():
    """`from fused_ssim import fused_ssim` (the reference's gaussian_splatting/utils/loss_utils.py:19) resolves to ours, with
    upstream's signature and defaults."""
    from fused_ssim import fused_ssim
    from monogs_amd import ssim
    assert fused_ssim is ssim.fused_ssim
    params = inspect.signature(fused_ssim).parameters
    assert list(params) == ["img1", "img2", "padding", "train"]
    assert params["img1"].default is inspect.Parameter.empty and params["img2"].default is inspect.Parameter.empty
    assert params["padding"].default == "same" and params["train"].default is True


def test_reference_call_sites_bind():
    from fused_ssim import fused_ssim
    lu = SEAM["loss_utils"]
    assert lu["imports_fused_ssim"] == ["fused_ssim"] and lu["module_level_import"]
    (call,) = lu["fused_ssim_calls"]
    assert call["n_args"] == 2 and call["keywords"] == {"padding": "valid"}
    sig = inspect.signature(fused_ssim)
    sig.bind(*[object()] * call["n_args"], **call["keywords"])            # the reference's call is accepted
    assert lu["ssim_params"] == [["img1", "img2"]]
    for key in ("slam_mapper", "eval_utils"):                             # ssim(image, gt_image): two positional tensors
        assert "ssim" in SEAM[key]["imports_loss_utils"]
        (c,) = SEAM[key]["ssim_calls"]
        assert c["n_args"] == 2 and not c["keywords"]
    # every config's lambda_ssim is the default of the fused refinement loss
    from monogs_amd import fused_losses
    assert SEAM["lambda_ssim"] and len(SEAM["lambda_ssim"]) >= 6
    default = inspect.signature(fused_losses.get_loss_refinement).parameters["lambda_ssim"].default
    assert all(v == default == 0.2 for v in SEAM["lambda_ssim"].values())
    assert inspect.signature(fused_losses.refinement_loss_grads).parameters["lambda_ssim"].default == 0.2


def test_header_declares_the_ssim_entry_points(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES and hasattr(native_lib, s)
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 12
    from monogs_amd import ssim
    c1 = float(re.search(r"#define MGS_SSIM_C1 ([0-9.]+)f", text).group(1))
    c2 = float(re.search(r"#define MGS_SSIM_C2 ([0-9.]+)f", text).group(1))
    assert abs(c1 - ssim.C1) < 1e-12 and abs(c2 - ssim.C2) < 1e-12 and abs(ssim.C1 - so.C1) < 1e-18


def test_scratch_size_is_pure_and_counts_the_planes(native_lib):
    lean, train = native_lib.mgs_ssim_scratch_bytes(3, 640, 480, 0), native_lib.mgs_ssim_scratch_bytes(3, 640, 480, 1)
    assert train - lean == 3 * 3 * 640 * 480 * 4          # three derivative planes per image plane, nothing else
    assert 64 <= lean < 64 * 1024
    assert native_lib.mgs_ssim_scratch_bytes(3, 640, 480, 1) == train


def test_entry_points_refuse_bad_arguments_before_any_launch(native_lib):
    """NULL pointers and "valid" under 11 pixels come back as argument errors (code 1) with a message; nothing is launched, so
    this runs without a device."""
    P = 0x1000                         # non-NULL and never dereferenced
    err = lambda: native_lib.mgs_last_error().decode()  # noqa: E731
    assert native_lib.mgs_ssim_forward(3, 64, 64, 0, 1, so.C1, so.C2, None, P, P, P, None) == 1 and "non-NULL" in err()
    assert native_lib.mgs_ssim_forward(3, 64, 64, 0, 1, so.C1, so.C2, P, P, None, P, None) == 1 and "non-NULL" in err()
    assert native_lib.mgs_ssim_forward(3, 64, 64, 0, 1, so.C1, so.C2, P, P, P, None, None) == 1 and "non-NULL" in err()
    assert native_lib.mgs_ssim_forward(3, 10, 64, 1, 1, so.C1, so.C2, P, P, P, P, None) == 1 and "11 x 11" in err()
    assert native_lib.mgs_ssim_forward(3, 64, 10, 1, 0, so.C1, so.C2, P, P, P, P, None) == 1 and "11 x 11" in err()
    assert native_lib.mgs_ssim_forward(0, 64, 64, 0, 1, so.C1, so.C2, P, P, P, P, None) == 1 and "positive" in err()
    assert native_lib.mgs_ssim_backward(3, 64, 64, 0, so.C1, so.C2, P, P, None, None, P, None) == 1 and "non-NULL" in err()
    assert native_lib.mgs_ssim_backward(3, 64, 64, 0, so.C1, so.C2, P, P, P, None, None, None) == 1 and "non-NULL" in err()
    assert native_lib.mgs_ssim_backward(3, 64, 5, 1, so.C1, so.C2, P, P, P, None, P, None) == 1 and "11 x 11" in err()
    assert native_lib.mgs_refine_loss_forward(64, 64, 0.2, None, P, P, P, None) == 1 and "non-NULL" in err()
    assert native_lib.mgs_refine_loss_forward(64, 64, 0.2, P, P, P, None, None) == 1 and "non-NULL" in err()
    assert native_lib.mgs_refine_loss_backward(64, 64, 0.2, P, P, P, None, None, None) == 1 and "non-NULL" in err()
    assert native_lib.mgs_refine_loss_grads(64, 64, 0.2, P, None, P, P, None) == 1 and "non-NULL" in err()
    assert native_lib.mgs_refine_loss_grads(64, 64, 0.2, P, P, P, None, None) == 1 and "non-NULL" in err()
    assert native_lib.mgs_refine_loss_grads(10, 64, 0.2, P, P, P, P, None) == 1 and "11 x 11" in err()
    assert native_lib.mgs_refine_loss_grads(64, 64, 1.5, P, P, P, P, None) == 1 and "lambda_ssim" in err()


def test_python_argument_errors(native_lib):
    from fused_ssim import fused_ssim
    from monogs_amd import fused_losses
    a, b = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_ssim(a, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_ssim(a[0], b[0], padding="valid", train=False)
    with pytest.raises(ValueError, match="padding"):
        fused_ssim(a, b, padding="reflect")
    with pytest.raises(ValueError, match="same shape"):
        fused_ssim(a, b[:, :, :8])
    with pytest.raises(ValueError, match="11 x 11"):
        fused_ssim(a[..., :10], b[..., :10], padding="valid")
    with pytest.raises(ValueError, match=r"\[B,C,H,W\]"):
        fused_ssim(a[0, 0], b[0, 0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_losses.get_loss_refinement(a[0], b[0])
    with pytest.raises(ValueError, match="11 x 11"):
        fused_losses.refinement_loss_grads(a[0, :, :10], b[0, :, :10])
    with pytest.raises(ValueError, match=r"\[3,H,W\]"):
        fused_losses.get_loss_refinement(a[0, :2], b[0, :2])


@pytest.mark.parametrize("kind,shape,padding", so.cases(), ids=lambda v: str(v).replace(" ", ""))
def test_checker_agrees_with_scipy(kind, shape, padding):
    """The conv2d checker against scipy.ndimage.correlate1d along both axes: two independent float64 evaluations."""
    a, b = so.make_pair(kind, shape)
    ref = float(so.ssim_ref(a, b, padding))
    alt = so.ssim_scipy(a.numpy(), b.numpy(), padding)
    assert abs(ref - alt) <= 5e-13, (ref, alt)
    if shape[-2] >= 480:                         # on the full-size images the classes are what they claim to be
        if kind == "smooth":
            assert 0.80 < ref < 0.99, ref
        elif kind == "noise":
            assert abs(ref) < 0.05, ref


def test_checker_identity_and_input_classes():
    for shape in ((1, 3, 37, 53), (1, 1, 5, 7)):
        a, _ = so.make_pair("smooth", shape)
        for padding in ("same", "valid") if shape[-2] >= 11 else ("same",):
            assert abs(float(so.ssim_ref(a, a, padding)) - 1.0) <= 1e-12
    assert len(so.cases()) == 3 * (6 + 5)
    a, b = so.make_pair("flat", (1, 3, 16, 300))
    assert a.dtype == torch.float32 and 0 <= float(a.min()) and float(a.max()) <= 1 and float(a.var()) < 1e-5
    a2, b2 = so.make_pair("flat", (1, 3, 16, 300))
    assert torch.equal(a, a2) and torch.equal(b, b2)          # seeded
