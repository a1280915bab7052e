"""blend_backward_s_kernel forms what a lane of the flush derives from its number (row, q, three LDS addresses, first pixel) once
per walk (bs_lane_consts, blend.hip); blend_backward_t_kernel (option "blend_bwd_transposed" = 1), the same accumulation in the
same order per batch, still re-derives them in every batch.  One 16 x 16 tile with 1, 3, 4, 5 and 9 Gaussians over one quadrant:
that quadrant's wave flushes a batch of fewer than four survivors, exactly four, and four (or eight) plus a remainder, so the
hoisted constants serve a full batch, a partial one and several in a row.  Ten-sum and six-sum (pose-only) variant, unsplit and
split launch (lists this short are not divided: the split instantiation walks them from the back alone).  The bar is that of
tests/test_gpu_parity.py::test_blend_backward_paths_agree: 1e-6 relative L2 per tensor, 1e-5 for the pose gradients."""
import pytest
import torch

from monogs_amd.debug import options
from monogs_amd.synthetic import make_scene, scene_settings

DEV = "cuda:0"
TILE = dict(W=16, H=16, fx=16.0, fy=16.0, cx=7.5, cy=7.5)


def _scene(n):
    """n Gaussians of ~1 px sigma centred on pixels (3..4, 3..4) of the upper-left 8 x 8 quadrant, at distinct depths."""
    sc = make_scene(n, TILE, seed=n, pose_tau=(0.0,) * 6)
    i = torch.arange(n, dtype=torch.float32)
    z = 1.0 + 0.1 * i
    px, py = 3.0 + 0.25 * (i % 4), 3.0 + 0.3 * (i % 3)
    pc = torch.stack([(px - TILE["cx"]) / TILE["fx"] * z, (py - TILE["cy"]) / TILE["fy"] * z, z], dim=1)
    means = ((pc - sc.t[None, :]) @ sc.R).contiguous()
    s = (1.0 * z / TILE["fx"])[:, None] * torch.tensor([[1.0, 1.3, 0.8]])
    return sc._replace(means3D=means, scales=s.contiguous(), opacities=torch.full((n, 1), 0.3))


def _run(lib, sc, pose_only, transposed, split):
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)
    inp = dict(means3D=sc.means3D, opacities=sc.opacities, colors_precomp=sc.colors, scales=sc.scales, rotations=sc.rotations)
    leaves = {k: (v.to(DEV).clone() if pose_only else v.to(DEV).clone().requires_grad_(True)) for k, v in inp.items()}
    theta = torch.zeros(3, device=DEV, requires_grad=True)
    rho = torch.zeros(3, device=DEV, requires_grad=True)
    m2 = torch.zeros_like(leaves["means3D"], requires_grad=not pose_only)
    with options(blend_bwd_transposed=transposed, blend_bwd_split=split):
        out = GaussianRasterizer(st)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"],
                                     colors_precomp=leaves["colors_precomp"], scales=leaves["scales"],
                                     rotations=leaves["rotations"], theta=theta, rho=rho)
        # (the split launch needs the forward's images: `out` stays alive across the backward)
        torch.autograd.backward([out[0], out[2]], [sc.grad_color.to(DEV), sc.grad_depth.to(DEV)])
        torch.cuda.synchronize()
    g = dict(theta=theta.grad.clone(), rho=rho.grad.clone())
    if not pose_only:
        g.update({k: v.grad.clone() for k, v in leaves.items()}, means2D=m2.grad.clone())
    return g, int((out[4] > 0).sum().item())            # n_touched: Gaussians that reached a pixel


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("pose_only", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_s_kernel_flush_matches_the_t_kernel(native_lib, n, pose_only, split):
    sc = _scene(n)
    a, seen = _run(native_lib, sc, pose_only, 2, split)
    b, _ = _run(native_lib, sc, pose_only, 1, 0)
    assert seen == n                                    # every Gaussian reached a pixel: n survivors in the quadrant's walk
    assert set(a) == set(b) and len(a) == (2 if pose_only else 8)
    for k in a:
        x, y = a[k].double(), b[k].double()
        assert y.norm() > 0, k
        rel = ((x - y).norm() / y.norm()).item()
        print(f"n={n} pose_only={pose_only} split={split} {k}: rel L2 {rel:.2e}")
        assert rel <= (1e-5 if k in ("theta", "rho") else 1e-6), (k, rel)
