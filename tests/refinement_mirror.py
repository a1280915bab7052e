"""TEST INFRASTRUCTURE: one iteration of the reference's ``Mapper.refinement`` (/root/reference/utils/slam_mapper.py:509-548)
restated in plain PyTorch on ordinary leaf tensors, for tests/test_gpu_refinement.py to hold ``monogs_amd.refinement.Refiner``
against (and for tools/refine_bench.py to time as "the plain torch loop").

Nothing fused is used except the rasteriser itself, through the public ``monogs_amd.renderer.render`` seam: the activations are
``F.normalize`` / ``torch.exp`` / ``torch.sigmoid`` under autograd, the loss is ``(1 - lambda) |image - gt|.mean() + lambda (1 -
SSIM_valid)`` with the differentiable float64 SSIM of tests/ssim_oracle.py (on the CPU, where that checker lives; ``ssim=`` takes
another differentiable SSIM), ONE backward, ``max_radii_2d`` by boolean indexing, ``torch.optim.Adam(eps=1e-15)`` and
``expon_lr(iteration)`` with the refinement's own count.  State handling (leaves, optimiser state, keyframe copies) is
``MirrorWindow``'s."""
import torch
import torch.nn.functional as F

from mapping_mirror import NAMES, MirrorWindow
from monogs_amd.gaussian_optim import expon_lr
from monogs_amd.renderer import render


def ssim_valid_float64_cpu(image, gt):
    from ssim_oracle import ssim_ref
    return ssim_ref(image.cpu(), gt.cpu(), "valid", torch.float64).to(image.device, torch.float32)


class MirrorRefinement(MirrorWindow):
    def __init__(self, intr, bg, lambda_ssim=0.2, lr_schedule=None, ssim=ssim_valid_float64_cpu):
        super().__init__(intr, bg, window_size=0, lr_schedule=lr_schedule)
        self.lambda_ssim, self.ssim = float(lambda_ssim), ssim
        self.iteration = 0                       # the refinement's own count (slam_mapper.py:509)

    def forward_backward(self, k):
        """slam_mapper.py:515-540 for keyframe ``k`` of the loaded keyframes.  Returns the render package and the loss terms."""
        vp = self.vps[k]
        xyz, rgb, opacity, scaling, rotation = self.params()
        pkg = render(vp, self.intr, xyz, F.normalize(rotation), torch.exp(scaling), torch.sigmoid(opacity), rgb, self.bg)
        image, gt = pkg["render"], vp.rgb
        l1 = torch.abs(image - gt).mean()
        ssim = self.ssim(image, gt)
        loss = (1.0 - self.lambda_ssim) * l1 + self.lambda_ssim * (1.0 - ssim)
        loss.backward()
        self.autograd_grads = [None if p.grad is None else p.grad.detach().clone() for p in self.params()]
        return pkg, dict(loss=loss.detach(), l1=l1.detach(), ssim=ssim.detach())

    @torch.no_grad()
    def statistics_and_step(self, pkg, gaussian_grads=None):
        """slam_mapper.py:541-548: ``max_radii_2d`` over the visible Gaussians, ``optimizer.step()``, ``zero_grad``,
        ``update_learning_rate(iteration)``.  ``gaussian_grads`` replaces the five autograd gradients before the step."""
        self.iteration += 1
        vis, radii = pkg["visibility_filter"], pkg["radii"]
        self.max_radii_2d[vis] = torch.max(self.max_radii_2d[vis], radii[vis].float())
        if gaussian_grads is not None:
            for p, g in zip(self.params(), gaussian_grads):
                p.grad = None if g is None else g.detach().clone()
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)
        if self.lr_schedule is not None:
            self.group("xyz")["lr"] = expon_lr(self.iteration, **self.lr_schedule)

    def iterate(self, k, gaussian_grads=None):
        pkg, terms = self.forward_backward(k)
        self.statistics_and_step(pkg, gaussian_grads)
        return pkg, terms


__all__ = ["MirrorRefinement", "NAMES", "ssim_valid_float64_cpu"]
