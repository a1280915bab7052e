"""``Refiner`` -- the colour-refinement loop that ends a run, driven over the fused pieces, optionally from a hipGraph.

Mirror of ``Mapper.refinement`` (/root/reference/utils/slam_mapper.py:502-548): per iteration draw one keyframe uniformly
(:510-514), render it from the activated map with the raw image as target -- no exposure correction, no depth term, no
opacity term (:515-535) -- ``(1 - lambda) L1 + lambda (1 - SSIM)`` (:536-539), ONE backward (:540), ``max_radii_2d`` over the
visible Gaussians (:542-545; ``xyz_gradient_accum`` and ``denom`` are NOT touched), Adam on the five Gaussian tensors (:546-547),
``update_learning_rate(iteration)`` with the REFINEMENT's own count 1..iters (:548: the xyz schedule restarts from ``lr_init``).
Poses and exposures take no step.

A sibling of ``WindowMapper`` (monogs_amd/mapping.py), not a mode of it.  The two share ``monogs_amd.map_step.MapStep``: the
activations, the leaves that cut the autograd graph behind them, the rasteriser call, and everything from the activations'
backward through ``GaussianAdam.step`` to the schedule on the device; the loss is ``fused_losses.refinement_loss_grads``.  The
keyframe order is drawn on the host BEFORE the loop (``self.sequence``): reproducible, and the same when a chunk has to be run again.

``use_graph=True``: ONE captured iteration serves every keyframe, the way ``TrackingGraph`` serves every frame -- a static slot
holds the image and the camera tensors, the chosen keyframe is copied into it before each replay.  The capture is made on one
stream with no side streams.  A captured forward renders with a fixed instance capacity, so before every capture one exact
no-grad forward per keyframe measures the instance counts and the maximum is reserved (``rasterizer.reserve_capacity``); a
capture serves at most ``max_replays_per_capture`` replays, then the counts are measured again (splats grow over 26 000
steps).  Before a chunk everything an iteration writes is copied aside; if the rasteriser reports a capacity overflow after the
chunk (instances were dropped: its images and gradients are wrong), the copies are restored and the SAME chunk of
``self.sequence`` runs again from a new capture with the doubled capacity.
"""
from __future__ import annotations

import random
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib, camera as cam, fused_losses, rasterizer as _rast
from .gaussian_map import GaussianMap
from .map_step import MapStep, rasterize
from ._launch import _device_guard, _stream


class _Buffers:
    """Static state of the iteration for one map size: everything a captured iteration points at."""

    def __init__(self, gmap: GaussianMap, intr):
        dev = gmap.device
        f32 = dict(dtype=torch.float32, device=dev)
        H, W = int(intr.height), int(intr.width)
        self.step = MapStep(gmap)       # the activated tensors, their raw gradients and the refinement's own iteration count
        self.P = P = self.step.P
        self.holder = torch.zeros(P, 3, requires_grad=True, **f32)      # render()'s screen-space gradient holder
        self.zero_depth = torch.zeros(1, H, W, **f32)                   # dL/ddepth: the loss has no depth term
        # zero pose deltas of the iteration's own: no viewpoint is touched
        self.theta, self.rho = torch.nn.Parameter(torch.zeros(3, **f32)), torch.nn.Parameter(torch.zeros(3, **f32))
        self.acc = torch.zeros(2, 3, **f32)                             # sums of (loss, L1, SSIM): first / last window
        self.sticky = torch.zeros(1, dtype=torch.int32, device=dev)     # status bits of every replay since the chunk began
        # the static viewpoint slot of the captured iteration
        self.rgb, self.R, self.T = torch.zeros(3, H, W, **f32), torch.eye(3, **f32), torch.zeros(3, **f32)
        self.cam3 = (torch.empty(4, 4, **f32), torch.empty(4, 4, **f32), torch.empty(3, **f32))
        self.rg = None                  # the loss record of the last iteration


class Refiner:
    iteration_total = 26000          # /root/reference/utils/slam_mapper.py:508

    def __init__(self, gmap: GaussianMap, intr, bg, lambda_ssim: float = 0.2, seed: int = 0, use_graph: bool = False,
                 max_replays_per_capture: int = 256, first_reserve_scale: float = 1.0):
        """``first_reserve_scale``: the FIRST capture reserves that share of the measured instance count (tests: < 1 makes the
        first chunk overflow and drives the redo)."""
        assert gmap.fused_adam, "Refiner drives the fused optimiser (GaussianAdam)"
        self.gmap, self.intr, self.bg = gmap, intr, bg
        self.lambda_ssim, self.seed, self.use_graph = float(lambda_ssim), int(seed), bool(use_graph)
        self.max_replays_per_capture = int(max_replays_per_capture)
        self.first_reserve_scale = float(first_reserve_scale)
        self.sequence: List[int] = []
        self.stats = dict(captures=0, replays=0, eager_iters=0, overflow_redos=0)
        self.keep_grads = False          # tests: clones of the five gradients of the last iteration
        self.last_grads = None
        self.last_radii = None           # radii of the last iteration's render (int32[P])
        self._graph = None
        self._graph_flags = None         # owner of the captured forward's status word (one handle per capture)
        self._buf = None
        self._vps: List = []
        self._iters = self._done = self._window = 0

    # ---- the keyframe order ---------------------------------------------------------------------------------------------
    @staticmethod
    def draw_sequence(n_keyframes: int, iters: int, seed: int) -> List[int]:
        """``random.randint(0, len(stack) - 1)`` per iteration (/root/reference/utils/slam_mapper.py:510-514), from a generator of
        its own."""
        rng = random.Random(seed)
        return [rng.randint(0, n_keyframes - 1) for _ in range(iters)]

    # ---- one iteration (eager, or the body of the capture) ---------------------------------------------------------------
    def _iteration(self, b, rgb, cam3):
        gmap = self.gmap
        b.step.activate()
        leaves = b.step.leaves()
        h = b.holder
        h.grad = b.theta.grad = b.rho.grad = None
        color, radii, depth, _ = rasterize(self.intr, self.bg, cam3, leaves, h, b.theta, b.rho)
        if torch.cuda.is_current_stream_capturing():
            # a forward rewrites its status word: the chunk's check must see an overflow of ANY replay, whichever keyframe it drew
            self._graph_flags.accumulate(b.sticky)
        rg = fused_losses.refinement_loss_grads(color, rgb, self.lambda_ssim)
        torch.autograd.backward([color, depth], [rg.d_render, b.zero_depth])
        b.rg, self.last_radii = rg, radii
        with _device_guard(gmap._xyz.device):
            # max_radii_2d[visible] = max(., radii[visible]) alone (slam_mapper.py:542-545): NULL for the other two statistics
            _lib.check(_lib.load().mgs_densify_stats(b.P, h.grad.data_ptr(), radii.data_ptr(), None, None,
                                                     gmap.max_radii_2d.data_ptr(), _stream()), "mgs_densify_stats")

        def keep_grads():
            if self.keep_grads:
                self.last_grads = [q.grad.clone() for q in gmap.params()]
        # (contiguous views of the rasteriser's one gradient allocation, read in place)
        b.step.apply([t.grad for t in leaves], keep_grads)

    def _account(self, b, i, iters, m):
        """Iteration i's (loss, L1, SSIM) into the running sums of the first / last ``m`` iterations, on the device."""
        if i < m:
            b.acc[0] += b.rg.scratch[:3]
        if i >= iters - m:
            b.acc[1] += b.rg.scratch[:3]

    def _iterate_eager(self, b, vp, i, iters, m):
        cam3 = cam.cached_camera_tensors(vp, vp.R, vp.T, self.intr.projection_matrix)
        self._iteration(b, vp.rgb, cam3)
        self._account(b, i, iters, m)
        self.stats["eager_iters"] += 1

    # ---- capacity, capture, snapshot -------------------------------------------------------------------------------------
    @torch.no_grad()
    def _measure(self, b, vps) -> int:
        """One exact no-grad forward per keyframe at the current map: the largest instance count."""
        gmap, key = self.gmap, (b.P, int(self.intr.width), int(self.intr.height))
        with _rast.exact_counts():
            b.step.activate()
            five = (gmap._xyz.detach(), gmap._rgb.detach(), b.step.opac, b.step.scales3, b.step.rot)
            most = 0
            for vp in vps:
                cam3 = cam.cached_camera_tensors(vp, vp.R, vp.T, self.intr.projection_matrix)
                rasterize(self.intr, self.bg, cam3, five, b.holder.detach(), None, None)
                most = max(most, int(_rast.capacity_hint(*key)))
        return most

    def _capture(self, b, vps, at_least: int = 0):
        W, H = int(self.intr.width), int(self.intr.height)
        scale = self.first_reserve_scale if self.stats["captures"] == 0 else 1.0
        _rast.reserve_capacity(b.P, W, H, max(int(self._measure(b, vps) * scale), int(at_least)))
        self.gmap.optimizer.zero_grad(set_to_none=True)
        g = torch.cuda.CUDAGraph()
        self._graph_flags = _rast.graph_flags()
        with self._graph_flags, torch.cuda.graph(g):   # one stream, no side streams; a memory pool of its own, released with the graph
            self._iteration(b, b.rgb, b.cam3)
        self._graph = g
        self.stats["captures"] += 1

    def _drop_graph(self):
        if self._graph_flags is not None:
            self._graph_flags.release()
        self._graph = self._graph_flags = None
        if self._buf is not None:
            self._buf.rg = None
        self.gmap.optimizer.zero_grad(set_to_none=True)

    def _state(self, b):
        """Everything an iteration writes."""
        opt = self.gmap.optimizer
        return [p.data for p in self.gmap.params()] + list(opt.exp_avg) + list(opt.exp_avg_sq) + \
               [opt.t_dev, opt.device_lrs(), b.step.iter_dev, self.gmap.max_radii_2d, b.acc]

    @torch.no_grad()
    def _replay_chunk(self, b, vps, i0, n, iters, m):
        b.sticky.zero_()
        for i in range(i0, i0 + n):
            vp = vps[self.sequence[i]]
            b.rgb.copy_(vp.rgb); b.R.copy_(vp.R); b.T.copy_(vp.T)
            cam.fused_camera_matrices(b.R, b.T, self.intr.projection_matrix, out=b.cam3)
            self._graph.replay()
            self._account(b, i, iters, m)
        self.stats["replays"] += n

    # ---- the loop ------------------------------------------------------------------------------------------------------------
    def begin(self, viewpoints: Sequence, iters: Optional[int] = None) -> None:
        """Draws the keyframe order and restarts the refinement's own iteration count (hence the xyz schedule).  ``refine`` is
        ``begin`` + ``run`` + ``finish``; ``step_eager`` runs the next iteration alone (tests compare it step by step)."""
        iters = self.iteration_total if iters is None else int(iters)
        self._vps = list(viewpoints)
        if not self._vps or iters <= 0:
            raise ValueError("refinement needs at least one keyframe and one iteration")
        self.sequence = self.draw_sequence(len(self._vps), iters, self.seed)
        self._iters, self._done, self._window = iters, 0, min(iters // 4, 1000)
        if self._buf is None or self._buf.P != len(self.gmap):
            self._drop_graph()
            self._buf = _Buffers(self.gmap, self.intr)
        self._buf.step.set_iteration(0)
        self._buf.acc.zero_()

    def step_eager(self) -> int:
        """The next iteration of the sequence, eagerly (exact-count forward).  Returns the index of the keyframe it used."""
        k = self.sequence[self._done]
        self._iterate_eager(self._buf, self._vps[k], self._done, self._iters, self._window)
        self._done += 1
        return k

    def run(self) -> None:
        b, vps, iters, m = self._buf, self._vps, self._iters, self._window
        if not (self.use_graph and torch.device(self.gmap.device).type == "cuda"):
            while self._done < iters:
                self.step_eager()
            return
        if self._done == 0:
            self.step_eager()           # the first iteration is eager: whatever loads lazily does so outside a capture
        W, H = int(self.intr.width), int(self.intr.height)
        while self._done < iters:
            i, n = self._done, min(iters - self._done, self.max_replays_per_capture)
            with torch.no_grad():
                snap = [t.clone() for t in self._state(b)]
            self._capture(b, vps)
            self._replay_chunk(b, vps, i, n, iters, m)
            if _rast.check_overflow():
                # instances were dropped somewhere in the chunk: back to its start, a capture with the capacity that
                # check_overflow() doubled (or what the keyframes measure now, if that is more), the same chunk again
                doubled = int(_rast.capacity_hint(b.P, W, H) or 0)
                with torch.no_grad():
                    for t, s in zip(self._state(b), snap):
                        t.copy_(s)
                self._drop_graph()
                self.stats["replays"] -= n
                self.stats["overflow_redos"] += 1
                self._capture(b, vps, at_least=doubled)
                self._replay_chunk(b, vps, i, n, iters, m)
                if _rast.check_overflow():
                    raise RuntimeError(f"binning capacity overflow in refinement iterations {i + 1}..{i + n} again after the "
                                       "capacity was doubled")
            self._done += n
            self._drop_graph()          # splats grow: the next chunk measures and captures again

    def finish(self) -> Dict:
        m = self._window
        means = self._buf.acc.cpu() / max(m, 1)                      # the ONE read-back
        self._drop_graph()
        if self.gmap.lr_schedule is not None:
            self.gmap.optimizer.sync_lrs_from_device()
        keys = ("loss", "l1", "ssim")
        return dict(iters=self._done, window=m, stats=dict(self.stats),
                    first=dict(zip(keys, means[0].tolist())) if m else None,
                    last=dict(zip(keys, means[1].tolist())) if m else None)

    def refine(self, viewpoints: Sequence, iters: Optional[int] = None) -> Dict:
        """``viewpoints``: every keyframe of the run (the reference's ``viewpoints_dict``).  Returns ``iters``, ``stats`` and the
        means of loss / L1 / SSIM over the first and the last ``window = min(iters // 4, 1000)`` iterations (None when that is
        zero), accumulated on the device and read once at the end."""
        self.begin(viewpoints, iters)
        try:
            self.run()
            return self.finish()
        finally:
            self._drop_graph()

    def close(self):
        """Releases the captured graph (with its memory pool), its overflow flags and the iteration's buffers."""
        self._drop_graph()
        self._buf = None
