"""The tracker (/root/reference/utils/slam_tracker.py:83-193): pose-only Adam (rot 0.003, trans 0.001, exposure 0.01 --
/root/reference/configs/mono/tum/base_config.yaml:46-48), at most ``max_iters`` iterations of render -> get_loss_tracking ->
backward -> step -> update_pose, left early when the retraction step is < 1e-4.  ``track_eager`` launches every iteration from
Python; ``TrackingGraph`` captures one iteration per map version in a hipGraph and replays it.  A monocular viewpoint
(``Viewpoint(sensor="monocular")``) is tracked with ``get_loss_tracking_rgb``, eagerly and under capture."""
from __future__ import annotations

import torch

from . import camera as cam
from . import fused_losses
from .frames import Viewpoint
from .map_step import render_map
from .pose_optim import PoseAdam
from .rasterizer import GaussianRasterizer
from .renderer import raster_settings


def track_eager(vp, intr, gmap, bg, max_iters: int) -> int:
    """Tracks ``vp`` (starting from the pose it holds) against ``gmap``; returns the iterations run."""
    opt = PoseAdam(vp, 0.003, 0.001, 0.01)
    loss_fn = fused_losses.get_loss_tracking_rgb if getattr(vp, "sensor", "depth") == "monocular" else fused_losses.get_loss_tracking
    n_it = 0
    for it in range(max_iters):
        pkg = render_map(vp, intr, gmap, bg)
        opt.zero_grad()
        loss = loss_fn(pkg["render"], pkg["depth"], pkg["opacity"], vp)
        loss.backward()
        n_it += 1
        with torch.no_grad():
            if opt.step_and_retract():
                break
    return n_it


class TrackingGraph:
    """The tracking iteration (render -> fused loss -> backward -> fused pose step) captured ONCE per map version
    in a hipGraph and replayed for every iteration of every frame tracked against that map.

    * The forward runs in capacity mode (no host sync); the Adam step count and a sticky convergence flag live on the
      device, so a replay that runs after convergence changes nothing.
    * The frame being tracked is copied into a static viewpoint whose buffers the graph points at; the map is constant
      during tracking, so its activations are evaluated once and it takes no gradient.
    * The convergence flag is read back through a pinned buffer after every replay (or one replay late, `lookahead`).
    Result: identical poses and iteration counts to the eager loop with its per-iteration `if converged: break`."""

    def __init__(self, proto: Viewpoint, intr, gmap, bg, exclusive: bool = False):
        from . import rasterizer as _r
        self._r = _r
        dev = proto.device
        with torch.no_grad():
            self.map = (gmap.get_xyz.detach(), gmap.get_rotation.detach(), gmap.get_scaling.detach(),   # [P,1]: isotropic
                        gmap.get_opacity.detach(), gmap.get_features.detach())
        self.n_gaussians = int(self.map[0].shape[0])
        self.monocular = getattr(proto, "sensor", "depth") == "monocular"      # the captured loss is this sensor's
        self.svp = Viewpoint(-1, torch.zeros_like(proto.rgb), torch.zeros_like(proto.depth) if self.monocular
                             else torch.ones_like(proto.depth), dev, sensor="monocular" if self.monocular else "depth")
        self.opt = PoseAdam(self.svp, 0.003, 0.001, 0.01, sticky=True)
        self.intr, self.bg = intr, bg
        self.flags = [torch.zeros(1, pin_memory=True) for _ in range(2)]
        self.events = [torch.cuda.Event() for _ in range(2)]
        self.graph = None
        self.zero2d = torch.zeros_like(self.map[0])
        # the static viewpoint's camera tensors: computed when a frame is loaded, then kept current by the pose step itself
        self.cam3 = (torch.empty(4, 4, device=dev), torch.empty(4, 4, device=dev), torch.empty(3, device=dev))
        self._load(proto)
        keep = (self.svp.R.clone(), self.svp.T.clone(), self.svp.exposure_a.data.clone(), self.svp.exposure_b.data.clone())
        # eager warm-up on a side stream (also records the capacity hint for this map size), then capture
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._iteration()
        torch.cuda.current_stream().wait_stream(s)
        self.opt.zero_grad()
        # two executable graphs of the same iteration, replayed alternately: launching a graph that is still running
        # waits for it, a second instance lets replay n+1 queue behind replay n (the ~30 us launch gap disappears).
        # `exclusive`: this process owns the device and the replays run one after the other on one stream, so the small sorts
        # may skip their ticket atomics (MGS_FLAG_EXCLUSIVE_DEVICE) -- NOT what a tracker beside a mapper process may assume.
        self.graphs = []
        self.graph_flags = _r.graph_flags()          # owner of the two captured forwards' status words, until close()
        for slot in range(2):
            self.opt.zero_grad()
            g = torch.cuda.CUDAGraph()
            with self.graph_flags, torch.cuda.graph(g), _r.exclusive_device(exclusive):
                self._iteration(host_flag=self.flags[slot])      # graph `slot` reports into its own pinned word
            self.graphs.append(g)
        self.graph = self.graphs[0]
        with torch.no_grad():          # undo the warm-up step
            self.svp.R.copy_(keep[0]); self.svp.T.copy_(keep[1])
            self.svp.exposure_a.data.copy_(keep[2]); self.svp.exposure_b.data.copy_(keep[3])

    def _iteration(self, host_flag=None):
        # render() without what tracking never reads: no screen-space gradient holder, no visibility filter
        xyz, rot, sca3, opa, col = self.map
        color, _, depth, opacity, _ = GaussianRasterizer(raster_settings(self.intr, self.bg, *self.cam3))(
            means3D=xyz, means2D=self.zero2d, opacities=opa, colors_precomp=col, scales=sca3, rotations=rot,
            theta=self.svp.cam_rot_delta, rho=self.svp.cam_trans_delta)
        self.opt.zero_grad()
        # loss value + upstream gradients in two launches, then the rasteriser's backward directly: no autograd node for
        # the scalar (its finalize kernel and the ones-fill of loss.backward() were two of the 25 launches of a replay)
        lg = fused_losses.loss_grads(color, depth, opacity, self.svp, tracking=True, rgb_only=self.monocular)
        lg.backward(color, depth, self.svp)
        self.opt.step_and_retract(sync=False, host_flag=host_flag, camera=(self.intr.projection_matrix,) + self.cam3)

    @torch.no_grad()
    def _load(self, vp: Viewpoint):
        s = self.svp
        if (getattr(vp, "sensor", "depth") == "monocular") != self.monocular:
            raise ValueError(f"this tracking graph was captured for a {s.sensor} viewpoint")
        s.rgb.copy_(vp.rgb); s.depth.copy_(vp.depth); s.mask.copy_(vp.mask); s.grad_mask.copy_(vp.grad_mask)
        s.R.copy_(vp.R); s.T.copy_(vp.T)
        s.exposure_a.data.copy_(vp.exposure_a.data); s.exposure_b.data.copy_(vp.exposure_b.data)
        s.cam_rot_delta.data.zero_(); s.cam_trans_delta.data.zero_()
        cam.fused_camera_matrices(s.R, s.T, self.intr.projection_matrix, out=self.cam3)
        self.opt.reset()
        for f in self.flags:          # (host words; nothing is in flight between two frames)
            f.zero_()

    def track(self, vp: Viewpoint, max_iters: int, lookahead: int = 1) -> int:
        """lookahead = 0: read the convergence flag after every replay (one 4-byte read-back per iteration).
        lookahead = 1: launch replay n before reading the flag of replay n-1 (hides the read-back; relies on the sticky
        flag making the surplus replay a no-op)."""
        self._load(vp)
        n_done = max_iters
        for n in range(max_iters):
            self.graphs[n & 1].replay()          # its pose step stores the convergence flag into self.flags[n & 1] (pinned)
            self.events[n & 1].record()
            m = n - lookahead
            if m >= 0:
                self.events[m & 1].synchronize()
                if float(self.flags[m & 1][0]) > 0.5:       # iteration m converged; any later replay was a no-op
                    n_done = m + 1
                    break
        torch.cuda.current_stream().synchronize()
        if self._r.check_overflow():
            raise RuntimeError("binning capacity overflow inside the captured tracking graph")
        with torch.no_grad():
            vp.R, vp.T = self.svp.R.clone(), self.svp.T.clone()
            vp.exposure_a.data.copy_(self.svp.exposure_a.data); vp.exposure_b.data.copy_(self.svp.exposure_b.data)
        return n_done

    def close(self):
        self.graph_flags.release()
        self.graph = None
        self.graphs = []
