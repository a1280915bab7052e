"""float64 checker for the fused SSIM (test infrastructure, CPU only), written from the published definition
(Wang, Bovik, Sheikh, Simoncelli 2004, with the constants and the window every 3DGS code base uses):

    g = normalised 11-tap Gaussian, sigma 1.5, as the 11 x 11 outer product, zero padding
    mu1 = g*x, mu2 = g*y, s11 = g*x^2 - mu1^2, s22 = g*y^2 - mu2^2, s12 = g*xy - mu1 mu2
    map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2)),  C1 = 0.01^2, C2 = 0.03^2

"same": mean of the map; "valid": mean of the map without its outer 5 pixels.  Differentiated by autograd.
``ssim_scipy`` is an independent evaluation (scipy.ndimage.correlate1d along both axes) that pins ``ssim_ref`` on the CPU.
Also here: the three seeded input classes and the shapes of the test matrix."""
import math

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
RADIUS = 5

SHAPES = [(1, 3, 680, 1200), (1, 3, 480, 640), (2, 1, 37, 53), (1, 3, 11, 11), (1, 3, 16, 300), (1, 1, 5, 7)]
CLASSES = ("smooth", "noise", "flat")


def cases():
    """(class, shape, padding): every class x shape x padding; the 5 x 7 image only under "same"."""
    return [(k, s, p) for k in CLASSES for s in SHAPES for p in ("same", "valid")
            if not (p == "valid" and (s[-1] < 11 or s[-2] < 11))]


def window(dtype=torch.float64):
    k = torch.arange(-RADIUS, RADIUS + 1, dtype=torch.float64)
    g = torch.exp(-k * k / (2.0 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def ssim_map(img1, img2):
    """The SSIM map [B,C,H,W] in the dtype of the inputs (11 x 11 grouped conv2d, zero padding)."""
    B, C, H, W = img1.shape
    g = window(img1.dtype)
    w2 = torch.outer(g, g)[None, None].repeat(C, 1, 1, 1)
    conv = lambda t: F.conv2d(t, w2, padding=RADIUS, groups=C)  # noqa: E731
    mu1, mu2 = conv(img1), conv(img2)
    s11 = conv(img1 * img1) - mu1 * mu1
    s22 = conv(img2 * img2) - mu2 * mu2
    s12 = conv(img1 * img2) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))


def ssim_ref(img1, img2, padding="same", dtype=torch.float64):
    """Mean SSIM as a 0-d tensor of ``dtype`` (differentiable with respect to img1)."""
    if img1.dim() == 3:
        img1, img2 = img1[None], img2[None]
    m = ssim_map(img1.to(dtype), img2.to(dtype))
    if padding == "valid":
        m = m[..., RADIUS:-RADIUS, RADIUS:-RADIUS]
    return m.mean()


def ssim_value_and_grad(img1, img2, padding, upstream=lambda s: s, dtype=torch.float64):
    """(value, loss, dloss/dimg1) with loss = upstream(ssim), all in ``dtype`` on the CPU."""
    x = img1.detach().cpu().to(dtype).requires_grad_(True)
    s = ssim_ref(x, img2.detach().cpu().to(dtype), padding, dtype)
    loss = upstream(s)
    (g,) = torch.autograd.grad(loss, x)
    return s.detach(), loss.detach(), g


def ssim_scipy(img1, img2, padding="same"):
    """The same number with scipy.ndimage.correlate1d(mode="constant") along both axes, float64 numpy."""
    from scipy.ndimage import correlate1d
    x, y = np.asarray(img1, dtype=np.float64), np.asarray(img2, dtype=np.float64)
    k = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    g = np.exp(-k * k / (2.0 * 1.5 ** 2))
    g /= g.sum()
    blur = lambda t: correlate1d(correlate1d(t, g, axis=-1, mode="constant", cval=0.0), g, axis=-2, mode="constant", cval=0.0)  # noqa: E731
    mu1, mu2 = blur(x), blur(y)
    s11, s22, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    if padding == "valid":
        m = m[..., RADIUS:-RADIUS, RADIUS:-RADIUS]
    return float(m.mean())


def make_pair(kind, shape, seed=0):
    """Seeded float32 image pair in [0, 1] of one of the three classes."""
    gen = torch.Generator().manual_seed(1000 * seed + 17 * CLASSES.index(kind) + sum(shape))
    B, C, H, W = shape
    randn = lambda: torch.randn(shape, generator=gen)  # noqa: E731
    if kind == "smooth":      # render-against-photo-like
        grid = torch.rand((B, C, H // 8 + 2, W // 8 + 2), generator=gen)
        base = F.interpolate(grid, size=(H, W), mode="bicubic", align_corners=False)
        a, b = base + 0.05 * randn(), base + 0.02 * randn()
    elif kind == "noise":     # two independent images
        a, b = torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    elif kind == "flat":      # variance ~1e-6 next to C2 = 9e-4: the cancellation case of g*x^2 - mu^2 in float32
        a, b = 0.70 + 1e-3 * randn(), 0.69 + 1e-3 * randn()
    else:
        raise ValueError(kind)
    return a.clamp(0, 1).float().contiguous(), b.clamp(0, 1).float().contiguous()


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def bars(kind, img1, img2, padding, upstream):
    """(value bar, gradient bar) against the float64 checker: BASELINE.json north_star's 1e-4 absolute and 1e-3 relative L2;
    for the flat class max(north_star, 3 x the float32 torch checker's own distance to float64 on the same input) -- a
    property of the reference evaluation, never of the kernel under test; the factor 3 covers the other summation order of a
    separable kernel."""
    v_bar, g_bar = 1e-4, 1e-3
    if kind == "flat":
        v64, _, g64 = ssim_value_and_grad(img1, img2, padding, upstream, torch.float64)
        v32, _, g32 = ssim_value_and_grad(img1, img2, padding, upstream, torch.float32)
        v_bar = max(v_bar, 3.0 * abs(float(v32) - float(v64)))
        g_bar = max(g_bar, 3.0 * rel_l2(g32, g64))
    assert math.isfinite(v_bar) and math.isfinite(g_bar)
    return v_bar, g_bar
