"""The Gauss-Newton tracker: per iteration render -> pose-tangent planes -> normal equations -> damped step + retraction, left when
the step is < 1e-4 -- the second-order counterpart of ``tracking.track_eager`` / ``tracking.TrackingGraph`` (the reference's
tracker, /root/reference/utils/slam_tracker.py:83-193, is first-order Adam on the same rows).  Opt-in: ``run_slam(tracker=
"gauss_newton")``; the default tracker stays Adam.  A by-product is the 6 x 6 information matrix of every tracked pose
(``PoseGaussNewton.information``).

``GN_DEFAULTS`` are the tuned starting values ("Pose tangents", records what was tried)."""
from __future__ import annotations

import torch

from . import camera as cam
from .frames import Viewpoint
from .map_step import render_map
from .pose_jacobian import NormalEquations, SYSTEM_DOUBLES, normal_equations, pose_jacobian
from .pose_optim import PoseGaussNewton
from .rasterizer import GaussianRasterizer
from .renderer import raster_settings

GN_DEFAULTS = dict(delta_rgb=0.05, delta_depth=0.05, lam=1e-3, lam_abs=0.0, max_rot=0.05, max_trans=0.05)


def _split(params):
    p = dict(GN_DEFAULTS, **params)
    return (dict(delta_rgb=p.pop("delta_rgb"), delta_depth=p.pop("delta_depth")), p)


def track_gauss_newton(vp, intr, gmap, bg, max_iters: int, **params) -> int:
    """Tracks ``vp`` (starting from the pose it holds) against ``gmap`` with Gauss-Newton steps; returns the iterations run.
    ``params`` override ``GN_DEFAULTS``.  ``vp.gn_information`` receives the information matrix of the last step."""
    deltas, step = _split(params)
    opt = PoseGaussNewton(vp, **step)
    mono = getattr(vp, "sensor", "depth") == "monocular"
    n_it = 0
    for _ in range(max_iters):
        pkg = render_map(vp, intr, gmap, bg)
        J = pose_jacobian(pkg["render"])
        system = normal_equations(J, pkg["render"], pkg["depth"], pkg["opacity"], vp, rgb_only=mono, **deltas)
        n_it += 1
        if opt.step_and_retract(system):
            break
    if n_it:
        vp.gn_information = opt.information()
    return n_it


class GaussNewtonGraph:
    """The Gauss-Newton iteration captured ONCE per map version in a hipGraph and replayed for every iteration of every frame
    tracked against that map -- ``TrackingGraph``'s discipline: one stream with no parallel branches, the forward in capacity
    mode, two executable instances replayed alternately, a sticky convergence flag reported into a pinned word per instance, the
    captured forwards' status words owned by a ``graph_flags`` handle until ``close()``, ``check_overflow`` after every frame.
    A monocular prototype captures the RGB-only rows."""

    def __init__(self, proto: Viewpoint, intr, gmap, bg, exclusive: bool = False, **params):
        from . import rasterizer as _r
        self._r = _r
        dev = proto.device
        self.deltas, step = _split(params)
        with torch.no_grad():
            self.map = (gmap.get_xyz.detach(), gmap.get_rotation.detach(), gmap.get_scaling.detach(),
                        gmap.get_opacity.detach(), gmap.get_features.detach())
        self.n_gaussians = int(self.map[0].shape[0])
        self.monocular = getattr(proto, "sensor", "depth") == "monocular"
        self.svp = Viewpoint(-1, torch.zeros_like(proto.rgb), torch.zeros_like(proto.depth) if self.monocular
                             else torch.ones_like(proto.depth), dev, sensor="monocular" if self.monocular else "depth")
        self.opt = PoseGaussNewton(self.svp, sticky=True, **step)
        self.intr, self.bg = intr, bg
        self.flags = [torch.zeros(1, pin_memory=True) for _ in range(2)]
        self.events = [torch.cuda.Event() for _ in range(2)]
        self.zero2d = torch.zeros_like(self.map[0])
        self.system = NormalEquations(torch.zeros(SYSTEM_DOUBLES, dtype=torch.float64, device=dev))
        self.steps = torch.zeros(1, dtype=torch.int32, device=dev)          # iterations that moved the pose (device count)
        self.cam3 = (torch.empty(4, 4, device=dev), torch.empty(4, 4, device=dev), torch.empty(3, device=dev))
        self._load(proto)
        keep = (self.svp.R.clone(), self.svp.T.clone(), self.svp.exposure_a.data.clone(), self.svp.exposure_b.data.clone())
        s = torch.cuda.Stream()              # eager warm-up on a side stream (records the capacity hint), then capture
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._iteration()
        torch.cuda.current_stream().wait_stream(s)
        self.graphs = []
        self.graph_flags = _r.graph_flags()
        for slot in range(2):
            g = torch.cuda.CUDAGraph()
            with self.graph_flags, torch.cuda.graph(g), _r.exclusive_device(exclusive):
                self._iteration(host_flag=self.flags[slot])
            self.graphs.append(g)
        with torch.no_grad():                # undo the warm-up step
            self.svp.R.copy_(keep[0]); self.svp.T.copy_(keep[1])
            self.svp.exposure_a.data.copy_(keep[2]); self.svp.exposure_b.data.copy_(keep[3])
            self.opt.reset(); self.steps.zero_()

    def _iteration(self, host_flag=None):
        xyz, rot, sca3, opa, col = self.map
        color, _, depth, opacity, _ = GaussianRasterizer(raster_settings(self.intr, self.bg, *self.cam3))(
            means3D=xyz, means2D=self.zero2d, opacities=opa, colors_precomp=col, scales=sca3, rotations=rot,
            theta=self.svp.cam_rot_delta, rho=self.svp.cam_trans_delta)
        J = pose_jacobian(color)
        normal_equations(J, color, depth, opacity, self.svp, rgb_only=self.monocular, out=self.system, **self.deltas)
        with torch.no_grad():                # the count of the steps taken: a sticky no-op replay adds nothing
            self.steps += (self.opt.out[0:1] < 0.5).to(torch.int32)
        self.opt.step_and_retract(self.system, sync=False, host_flag=host_flag, camera=(self.intr.projection_matrix,) + self.cam3)

    @torch.no_grad()
    def _load(self, vp: Viewpoint):
        s = self.svp
        if (getattr(vp, "sensor", "depth") == "monocular") != self.monocular:
            raise ValueError(f"this tracking graph was captured for a {s.sensor} viewpoint")
        s.rgb.copy_(vp.rgb); s.depth.copy_(vp.depth); s.mask.copy_(vp.mask); s.grad_mask.copy_(vp.grad_mask)
        s.R.copy_(vp.R); s.T.copy_(vp.T)
        s.exposure_a.data.copy_(vp.exposure_a.data); s.exposure_b.data.copy_(vp.exposure_b.data)
        cam.fused_camera_matrices(s.R, s.T, self.intr.projection_matrix, out=self.cam3)
        self.opt.reset()
        self.steps.zero_()
        for f in self.flags:
            f.zero_()

    def track(self, vp: Viewpoint, max_iters: int, lookahead: int = 1) -> int:
        """As ``TrackingGraph.track``: replays until the flag of replay ``n - lookahead`` is up; returns the iterations run."""
        self._load(vp)
        n_done = max_iters
        for n in range(max_iters):
            self.graphs[n & 1].replay()
            self.events[n & 1].record()
            m = n - lookahead
            if m >= 0:
                self.events[m & 1].synchronize()
                if float(self.flags[m & 1][0]) > 0.5:
                    n_done = m + 1
                    break
        torch.cuda.current_stream().synchronize()
        if self._r.check_overflow():
            raise RuntimeError("binning capacity overflow inside the captured tracking graph")
        with torch.no_grad():
            vp.R, vp.T = self.svp.R.clone(), self.svp.T.clone()
            vp.exposure_a.data.copy_(self.svp.exposure_a.data); vp.exposure_b.data.copy_(self.svp.exposure_b.data)
            vp.gn_information = self.opt.information()
        return n_done

    def close(self):
        self.graph_flags.release()
        self.graphs = []
