"""Host side of the feature render (monogs_amd/feature_render.py): every shape, dtype and device error is raised in Python
before the library is touched, and header, library and binding agree on ABI v17.  No GPU needed: the rasteriser forward behind
``color`` is stood in for by an autograd Function that carries what ``render_features`` looks for on ``grad_fn``."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, H, W = 10, 12, 20


class _FakeForward(torch.autograd.Function):
    """A node ``rasterizer.forward_scratch`` accepts: what ``_RasterizeGaussians.forward`` leaves on its own ctx (raster_settings,
    cam, keep, offsets, the count, its saved tensors), with placeholders for every tensor."""

    @staticmethod
    def forward(ctx, colors):
        from monogs_amd import _lib
        from monogs_amd.rasterizer import GaussianRasterizationSettings
        z = torch.zeros(1)
        ctx.raster_settings = GaussianRasterizationSettings(H, W, 1.0, 1.0, torch.zeros(3), 1.0, z, z, z, 0, z, False, False)
        ctx.cam, ctx.keep, ctx.geom_off, ctx.img_off, ctx.num_rendered = _lib.MgsCamera(), [], 0, 256, 0
        ctx.save_for_backward(torch.zeros(P, 3), *[torch.zeros(1) for _ in range(7)], torch.zeros(512, dtype=torch.uint8),
                              torch.zeros(256, dtype=torch.uint8))
        return torch.zeros(3, H, W)

    @staticmethod
    def backward(ctx, g):
        return torch.zeros(P, 3)


@pytest.fixture
def color(monkeypatch):
    from monogs_amd import _lib

    def no_library():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    return _FakeForward.apply(torch.zeros(P, 3, requires_grad=True))


def test_exports():
    import monogs_amd
    from monogs_amd import FeatureRasterizer, render_features
    from monogs_amd import feature_render
    assert render_features is feature_render.render_features and FeatureRasterizer is feature_render.FeatureRasterizer
    assert monogs_amd.feature_render.MAX_FEATURE_CHANNELS == 256


@pytest.mark.parametrize("K", [0, 257])
def test_channel_count_outside_1_256(color, K):
    from monogs_amd import render_features
    with pytest.raises(ValueError, match="1..256 channels"):
        render_features(color, torch.zeros(P, K))


def test_features_shape_and_dtype(color):
    from monogs_amd import render_features
    with pytest.raises(ValueError, match=r"\[P, K\]"):
        render_features(color, torch.zeros(P, 4, 1))
    with pytest.raises(ValueError, match=r"\[P, K\]"):
        render_features(color, torch.zeros(P))
    with pytest.raises(ValueError, match="11 rows"):
        render_features(color, torch.zeros(P + 1, 4))
    with pytest.raises(TypeError, match="float32"):
        render_features(color, torch.zeros(P, 4, dtype=torch.float64))
    with pytest.raises(TypeError, match="float32"):
        render_features(color, torch.zeros(P, 4, dtype=torch.int32))


def test_color_must_come_from_the_rasteriser(color):
    from monogs_amd import render_features
    feats = torch.zeros(P, 4)
    for c in (torch.zeros(3, H, W), torch.zeros(3, H, W, requires_grad=True) * 2.0, color.detach()):
        with pytest.raises(RuntimeError, match="differentiable rasteriser forward"):
            render_features(c, feats)


def test_background_length_dtype_device(color):
    from monogs_amd import render_features
    feats = torch.zeros(P, 4)
    for bg in (torch.zeros(3), torch.zeros(5), torch.zeros(4, 1)):
        with pytest.raises(ValueError, match="bg must have K = 4"):
            render_features(color, feats, bg=bg)
    with pytest.raises(TypeError, match="bg must be float32"):
        render_features(color, feats, bg=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="is on meta"):
        render_features(color, torch.zeros(P, 4, device="meta"))


def test_valid_arguments_reach_the_library(color):
    """The stand-in passes every check: what stops a valid call is the library stub, nothing earlier."""
    from monogs_amd import render_features
    with pytest.raises(AssertionError, match="library was touched"):
        render_features(color, torch.zeros(P, 4), bg=torch.zeros(4))


def test_header_library_and_binding_agree_on_v17(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 17
    assert native_lib.mgs_abi_version() == _lib.ABI_VERSION
    assert re.search(r"#define MGS_MAX_FEATURE_CHANNELS 256\b", text)
    for name in ("mgs_features_forward", "mgs_features_backward"):
        assert re.search(r"\bint %s\(const mgs_camera\* cam, int32_t P, int32_t K, uint64_t num_rendered," % name, text), name
        assert name in _lib.SIGNATURES and hasattr(native_lib, name)


def test_library_refuses_bad_channel_counts_and_oversized_maps(native_lib):
    """K outside 1..256 and P > MGS_MAX_GAUSSIANS come back as argument errors before anything is launched (no GPU needed)."""
    import ctypes
    from monogs_amd import _lib
    cam = _lib.MgsCamera()
    cam.image_height, cam.image_width = 16, 16
    for f in ("bg", "viewmatrix", "projmatrix", "projmatrix_raw", "campos"):
        setattr(cam, f, 0x1000)                      # non-NULL and never dereferenced: the checks come first
    fwd = lambda P_, K_: native_lib.mgs_features_forward(ctypes.byref(cam), P_, K_, 1, *[None] * 7, 0.5, None)  # noqa: E731
    bwd = lambda P_, K_: native_lib.mgs_features_backward(ctypes.byref(cam), P_, K_, 1, *[None] * 5, None)  # noqa: E731
    for call in (fwd, bwd):
        for K in (0, 257, -1):
            assert call(8, K) == 1
            assert b"MGS_MAX_FEATURE_CHANNELS" in native_lib.mgs_last_error()
        assert call(1 << 26, 4) == 1
        assert b"MGS_MAX_GAUSSIANS" in native_lib.mgs_last_error()
