"""Fused SSIM and the fused refinement loss on the GPU (pytest -m gpu) against the float64 checker of tests/ssim_oracle.py.

Bars (BASELINE.json north_star): value 1e-4 absolute, gradient 1e-3 relative L2 per tensor; for the flat class
max(north_star, 3 x the float32 torch checker's own distance to float64 on the same input) -- see ssim_oracle.bars."""
import pytest
import torch

import ssim_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UP = lambda s: 3.7 * 0.2 * (1.0 - s)  # noqa: E731  (a non-unit upstream gradient)


def _pair(kind, shape, seed=0):
    a, b = so.make_pair(kind, shape, seed)
    return a.to(DEV), b.to(DEV)


@pytest.mark.parametrize("kind,shape,padding", so.cases(), ids=lambda v: str(v).replace(" ", ""))
def test_value_and_gradient_against_float64(native_lib, kind, shape, padding):
    from fused_ssim import fused_ssim
    a_cpu, b_cpu = so.make_pair(kind, shape)
    x = a_cpu.to(DEV).requires_grad_(True)
    val = fused_ssim(x, b_cpu.to(DEV), padding=padding)
    assert val.dim() == 0 and val.dtype == torch.float32 and val.device == x.device
    UP(val).backward()
    v64, _, g64 = so.ssim_value_and_grad(a_cpu, b_cpu, padding, UP)
    v_bar, g_bar = so.bars(kind, a_cpu, b_cpu, padding, UP)
    v_err, g_err = abs(float(val.detach()) - float(v64)), so.rel_l2(x.grad, g64)
    print(f"ssim {kind} {shape} {padding}: value {float(v64):.6f} err {v_err:.2e} (bar {v_bar:.1e}); "
          f"grad rel L2 {g_err:.2e} (bar {g_bar:.1e})")
    assert x.grad.shape == x.shape and torch.isfinite(x.grad).all()
    assert v_err <= v_bar, (v_err, v_bar)
    assert g_err <= g_bar, (g_err, g_bar)


def test_interface_equivalences_are_bitwise(native_lib):
    from fused_ssim import fused_ssim
    a, b = _pair("smooth", (1, 3, 37, 53))
    for padding in ("same", "valid"):
        # img2 takes no gradient
        x, y = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        v = fused_ssim(x, y, padding=padding)
        v.backward()
        assert y.grad is None and x.grad is not None
        # [C,H,W] is one image
        x3 = a[0].clone().requires_grad_(True)
        v3 = fused_ssim(x3, b[0], padding=padding)
        v3.backward()
        assert torch.equal(v3, v) and torch.equal(x3.grad, x.grad[0]) and x3.grad.shape == (3, 37, 53)
        # train=False: same value, nothing to differentiate
        vt = fused_ssim(a.clone().requires_grad_(True), b, padding=padding, train=False)
        assert torch.equal(vt, v) and not vt.requires_grad
        assert not fused_ssim(a, b, padding=padding).requires_grad and torch.equal(fused_ssim(a, b, padding=padding), v)
    # channel-sliced and transposed (non-contiguous) inputs equal their contiguous copies
    big_a, big_b = _pair("smooth", (1, 5, 53, 37))
    xs = big_a.clone().requires_grad_(True)
    sl_a, sl_b = xs[:, 1:4].transpose(2, 3), big_b[:, 1:4].transpose(2, 3)
    assert not sl_a.is_contiguous()
    v1 = fused_ssim(sl_a, sl_b, padding="valid")
    v1.backward()
    xc = sl_a.detach().contiguous().requires_grad_(True)
    v2 = fused_ssim(xc, sl_b.contiguous(), padding="valid")
    v2.backward()
    assert torch.equal(v1, v2) and torch.equal(xs.grad[:, 1:4].transpose(2, 3), xc.grad)
    assert float(xs.grad[:, 0].abs().max()) == 0.0 and float(xs.grad[:, 4].abs().max()) == 0.0


def test_reproducible_bitwise(native_lib):
    from fused_ssim import fused_ssim
    a, b = _pair("noise", (1, 3, 480, 640))
    runs = []
    for _ in range(2):
        x = a.clone().requires_grad_(True)
        v = fused_ssim(x, b, padding="valid")
        UP(v).backward()
        runs.append((v.detach().clone(), x.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_two_forwards_before_two_backwards_and_retain_graph(native_lib):
    """The mapper renders a window before it backpropagates (the reference's utils/slam_mapper.py:273-394): every forward owns
    its derivative planes."""
    from fused_ssim import fused_ssim
    a1, b1 = _pair("smooth", (1, 3, 37, 53), seed=1)
    a2, b2 = _pair("noise", (1, 3, 37, 53), seed=2)
    alone = []
    for a, b in ((a1, b1), (a2, b2)):
        x = a.clone().requires_grad_(True)
        fused_ssim(x, b, padding="valid").backward()
        alone.append(x.grad.clone())
    x1, x2 = a1.clone().requires_grad_(True), a2.clone().requires_grad_(True)
    v1 = fused_ssim(x1, b1, padding="valid")
    v2 = fused_ssim(x2, b2, padding="valid")
    v1.backward(retain_graph=True)
    v2.backward()
    assert torch.equal(x1.grad, alone[0]) and torch.equal(x2.grad, alone[1])
    first = x1.grad.clone()
    x1.grad = None
    v1.backward()                                      # a second backward through the same forward
    assert torch.equal(x1.grad, first)


def _torch_refinement(image, gt, lam, ssim_fn):
    return (1.0 - lam) * (image - gt).abs().mean() + lam * (1.0 - ssim_fn(image, gt))


@pytest.mark.parametrize("shape", [(3, 480, 640), (3, 37, 53), (3, 11, 11)])
def test_refinement_loss(native_lib, shape):
    from fused_ssim import fused_ssim
    from monogs_amd import fused_losses as F
    lam = 0.2
    a_cpu, b_cpu = so.make_pair("smooth", (1,) + shape, seed=3)
    a, b = a_cpu[0].to(DEV), b_cpu[0].to(DEV)
    x = a.clone().requires_grad_(True)
    loss = F.get_loss_refinement(x, b, lam)
    (1.9 * loss).backward()
    composed = _torch_refinement(a, b, lam, lambda i, g: fused_ssim(i, g, padding="valid"))
    assert abs(float(loss) - float(composed)) <= 1e-6 * abs(float(composed)), (float(loss), float(composed))
    x64 = a_cpu[0].double().requires_grad_(True)
    l64 = _torch_refinement(x64, b_cpu[0].double(), lam, lambda i, g: so.ssim_ref(i, g, "valid"))
    (g64,) = torch.autograd.grad(1.9 * l64, x64)
    err = so.rel_l2(x.grad, g64)
    print(f"refinement loss {shape}: value {float(loss):.6f} (float64 {float(l64):.6f}), grad rel L2 {err:.2e}")
    assert abs(float(loss) - float(l64)) <= 1e-4 and err <= 1e-3
    # value + gradient without an autograd node: the autograd path with grad_output = 1, bit for bit
    x1 = a.clone().requires_grad_(True)
    l1 = F.get_loss_refinement(x1, b, lam)
    l1.backward()
    rg = F.refinement_loss_grads(a, b, lam)
    assert rg.d_render.shape == a.shape
    assert torch.equal(rg.loss, l1.detach()) and torch.equal(rg.d_render, x1.grad)
    assert abs(float(rg.l1) - float((a - b).abs().mean())) <= 1e-6
    assert torch.equal(rg.ssim, fused_ssim(a, b, padding="valid"))
    assert abs(float(rg.loss) - ((1 - lam) * float(rg.l1) + lam * (1 - float(rg.ssim)))) <= 1e-6


def test_refinement_loss_grads_replays_from_a_graph(native_lib):
    from monogs_amd import fused_losses as F
    shape = (1, 3, 120, 200)
    contents = [_pair("smooth", shape, seed=s) for s in (4, 5, 6)]
    s_img, s_gt = torch.zeros(shape[1:], device=DEV), torch.zeros(shape[1:], device=DEV)
    s_img.copy_(contents[0][0][0]); s_gt.copy_(contents[0][1][0])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        F.refinement_loss_grads(s_img, s_gt, 0.2)                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        rg = F.refinement_loss_grads(s_img, s_gt, 0.2)
    for a, b in contents:
        s_img.copy_(a[0]); s_gt.copy_(b[0])
        graph.replay()
        torch.cuda.synchronize()
        eager = F.refinement_loss_grads(a[0], b[0], 0.2)
        assert torch.equal(rg.loss, eager.loss) and torch.equal(rg.d_render, eager.d_render)
        assert torch.equal(rg.l1, eager.l1) and torch.equal(rg.ssim, eager.ssim)


def test_end_to_end_refinement_step_against_the_oracle_chain(native_lib):
    """HIP render -> fused refinement loss -> HIP backward, against the oracle rasteriser fed the float64 checker's gradient at
    the oracle's own image: the bar and the form of __graft_entry__.smoke() and of the C2 chain in tests/test_gpu_parity.py."""
    from monogs_amd import fused_losses as F
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from monogs_amd.synthetic import make_scene, scene_settings
    from oracle import OracleSettings, rasterize_autograd

    lam = 0.2
    sc = make_scene(2000, "fr3_office", seed=3)
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
    means, opac, col, rot = leaf(sc.means3D), leaf(sc.opacities), leaf(sc.colors), leaf(sc.rotations)
    scales = leaf(sc.scales.repeat(1, 3))
    means2D = torch.zeros_like(means, requires_grad=True)
    theta = torch.zeros(3, device=DEV, requires_grad=True)
    rho = torch.zeros(3, device=DEV, requires_grad=True)
    color, radii, depth, opacity, n_touched = GaussianRasterizer(st)(
        means3D=means, means2D=means2D, opacities=opac, colors_precomp=col, scales=scales, rotations=rot,
        theta=theta, rho=rho)
    H, W = color.shape[-2:]
    target = so.make_pair("smooth", (1, 3, H, W), seed=7)[1][0]            # a fixed seeded "photo"
    loss = F.get_loss_refinement(color, target.to(DEV), lam)
    loss.backward()

    inp = dict(means3D=sc.means3D, opacities=sc.opacities, colors_precomp=sc.colors, scales=sc.scales.repeat(1, 3),
               rotations=sc.rotations)
    ost = scene_settings(sc, OracleSettings)
    zero_c, zero_d = torch.zeros(3, H, W), torch.zeros(1, H, W)
    oout, _ = rasterize_autograd(inp, ost, zero_c, zero_d, dtype=torch.float32)
    assert (color.detach().cpu() - oout.color).abs().max() <= 1e-4
    img64 = oout.color.double().requires_grad_(True)
    l64 = _torch_refinement(img64, target.double(), lam, lambda i, g: so.ssim_ref(i, g, "valid"))
    (g_color,) = torch.autograd.grad(l64, img64)
    assert abs(float(loss) - float(l64)) <= 1e-4
    _, og = rasterize_autograd(inp, ost, g_color, zero_d, dtype=torch.float32)
    got = dict(means3D=means.grad, colors_precomp=col.grad, opacities=opac.grad, theta=theta.grad, rho=rho.grad)
    rep = {k: so.rel_l2(v.reshape(og[k].shape), og[k]) for k, v in got.items()}
    print("refinement step, HIP chain vs oracle chain, relative L2:", {k: f"{v:.2e}" for k, v in rep.items()})
    assert all(v < 1e-3 for v in rep.values()), rep
