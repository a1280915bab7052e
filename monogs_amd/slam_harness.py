"""The two run loops that measure the SLAM-level metric (tracking / mapping FPS, BASELINE.json configs 3-4) without the
reference's viewer and queues: ``run_slam`` in one process, ``run_slam_two_process`` with the reference's tracker / mapper split.

Only the order of the calls, as the tracker and ``Mapper.run`` make them (/root/reference/utils/slam_tracker.py:83-193,412-452,
utils/slam_mapper.py:639-722), the time brackets around them and the result dict: what they call lives in ``frames``, ``tracking``,
``mapping``, ``keyframe_window``, ``refinement``, ``evaluation``, ``sequences``, ``dataset`` and ``eager_probe``."""
from __future__ import annotations

import gc
import queue
import time
from contextlib import contextmanager
from types import SimpleNamespace
from typing import List

import torch

from .frames import Viewpoint, position_error
from .gaussian_map import GaussianMap
from .map_arena import MapArena
from .map_step import render_map
from .mapping import WindowMapper
from .monocular import is_monocular, monocular_frames, pseudo_depth, valid_rgb
from .sequences import make_room_sequence, make_sequence      # make_sequence: re-exported, bench.py imports it (and run_slam) from here
from .gn_tracking import GaussNewtonGraph, track_gauss_newton
from .tracking import TrackingGraph, track_eager


def _clock():
    torch.cuda.synchronize()
    return time.perf_counter()


@contextmanager
def _timed(stats, key, t0=None):
    """Adds the time of the block, taken between two device synchronisations, to ``stats[key]``.  With ``t0`` the bracket was
    opened earlier by ``_clock()`` and only closes here.  Yields the opening time."""
    t0 = _clock() if t0 is None else t0
    yield t0
    stats[key] += _clock() - t0


def _render_frozen(vp, intr, gmap, bg):
    with torch.no_grad():
        return render_map(vp, intr, gmap, bg)


def _slide_window(window, vp, window_size):
    """The interval policy: the new keyframe joins, the second-oldest leaves a full window (the first one anchors the map)."""
    window.append(vp)
    if len(window) > window_size:
        window.pop(1)


def _setup(c):
    """The state of a run: sequence, map, mapper, optional keyframe window, counters.  ``sequence``: a ``(frames, intr)`` pair (e.g.
    ``dataset.dataset_frames``) instead of a synthetic ``scene``: "room" = ray-cast opaque surfaces (survive the reference's pruning,
    carry ``segmentation`` for a map with ``nr_objects`` scores per Gaussian), "cloud" = ``make_sequence`` (historical).
    ``reference_lrs`` / ``map_surgery``: the reference's learning rates / densify, prune and opacity-reset schedule.
    ``kf_selection="overlap"``: a ``KeyframeWindow``, ``check_viewpoints_overlap`` being the tracker's flag (False in the fork).
    ``sensor="monocular"``: the frames carry no depth (a synthetic or RGB-D sequence is stripped of it, a monocular ``sequence`` is
    taken as it is); the tracker and the mapper then run the RGB-only losses and ``_map_keyframe`` back-projects depth hypotheses.
    ``learn_objects=N`` (needs ``nr_objects``): the map's object rows are learned, N iterations of ``ObjectLayerTrainer`` over the
    window after every mapping call (``_learn_objects``)."""
    from .gaussian_map import REFERENCE_LRS, REFERENCE_LR_SCHEDULE
    if c.learn_objects and c.nr_objects is None:
        raise ValueError("learn_objects needs nr_objects")
    if c.sensor not in ("depth", "monocular"):
        raise ValueError('sensor must be "depth" or "monocular"')
    if c.kf_selection not in ("interval", "overlap"):
        raise ValueError('kf_selection must be "interval" or "overlap"')
    if c.tracker not in ("adam", "gauss_newton"):
        raise ValueError('tracker must be "adam" or "gauss_newton"')
    if c.viewer_dir is not None:
        from .viewer import MODES
        c.viewer_modes = tuple(c.viewer_modes)
        if [m for m in c.viewer_modes if m not in MODES]:
            raise ValueError(f"viewer_modes must be among {MODES}")
        if "segmentation" in c.viewer_modes and c.nr_objects is None:
            raise ValueError("the segmentation mode needs nr_objects")
    if c.prune_after_mapping is None:
        c.prune_after_mapping = bool(c.map_surgery)
    if c.sequence is not None:
        frames, intr = c.sequence
    elif c.scene == "room":
        frames, intr = make_room_sequence(c.n_frames, c.intrinsics, device=c.device, with_segmentation=c.nr_objects is not None)
    else:
        frames, intr = make_sequence(c.n_frames, c.intrinsics, c.n_gaussians, device=c.device)
    if c.sensor == "monocular":
        if not all(is_monocular(f) for f in frames):
            frames = monocular_frames(frames)
    elif any(is_monocular(f) for f in frames):
        raise ValueError('the sequence holds monocular frames: run it with sensor="monocular"')
    # ``reference_densify``: new Gaussians as the fork hard-codes them (1/32 of the pixels at initialisation, 1/64 per keyframe, the
    # reference's point-size rule) instead of ``init_downsample`` / ``kf_downsample`` / ``point_size``
    if c.reference_densify:
        c.extend_kw = lambda init: dict(downsample=32 if init else 64, point_size=None)
    else:
        c.extend_kw = lambda init: dict(downsample=c.init_downsample if init else c.kf_downsample, point_size=c.point_size)
    bg = torch.zeros(3, device=c.device)
    gmap = GaussianMap(c.device, nr_objects=c.nr_objects, **(dict(learn_objects=True) if c.learn_objects else {}),
                       **(dict(lrs=REFERENCE_LRS) if c.reference_lrs else {}))
    if c.reference_lrs:
        gmap.lr_schedule = dict(REFERENCE_LR_SCHEDULE)
    gmap.surgery_log = []
    mapper = WindowMapper(gmap, intr, bg, window_size=c.window_size, use_graph=c.graph_mapping)
    mapper.map_surgery = bool(c.map_surgery)
    mapper.time_replays = True
    kfw = None
    if c.kf_selection == "overlap":
        from .keyframe_window import KeyframeWindow
        kfw = KeyframeWindow(c.window_size, check_viewpoints_overlap=c.check_viewpoints_overlap, kf_interval=c.kf_interval)
    return SimpleNamespace(
        c=c, frames=frames, intr=intr, bg=bg, gmap=gmap, mapper=mapper, kfw=kfw, window=[], tgraph=None,
        kf_list=[],                                     # every keyframe of the run (the reference's viewpoints_dict / kf_indices)
        pseudo_depth_stats=[],                          # monocular: (frame, median, std, count, used_init_rule) per keyframe
        per_frame=[], map_loss=[], window_sizes=[],     # (frame, tracking iterations); (first, last) mapping loss per call
        size_trace=[],                                  # (frame, Gaussians in the map after that keyframe's mapping)
        stats=dict(kf_extend_s=0.0, track_capture_s=0.0, track_s=0.0, track_iters=0, tracked=0, map_s=0.0, map_iters=0,
                   keyframes=0, renders=0),
        stats_kf=dict(keyframes_selected=0, evicted_by_cutoff=0, evicted_by_size=0),
        viewer=None, viewer_files=[],                   # ``viewer_dir``: the HeadlessViewer of the run and the PNGs it wrote
        obj_trainer=None, obj_loss=[])                  # ``learn_objects``: the trainer of the run, (first, last) loss per call


def _map_window(s, iters, init=False):
    """One ``Mapper`` keyframe: fresh keyframe optimisers, the optimisation call (split in 1 + ``iters - 1`` to record the first
    loss), then ``optimize_map(prune=True, iters=1)`` (``prune_after_mapping``; default: with ``map_surgery``)."""
    mapper, window = s.mapper, s.window
    it0 = mapper.nr_iters
    if init:
        mapper.initialize_map(window[0], iters=1)
        first = mapper.last_loss
        if iters > 1:
            mapper.initialize_map(window[0], iters=iters - 1)
    else:
        mapper.new_keyframe_optimizers(window)
        mapper.optimize_map(window, iters=1)
        first = mapper.last_loss
        if iters > 1:
            mapper.optimize_map(window, iters=iters - 1)
    last = mapper.last_loss
    if not init and s.c.prune_after_mapping:
        mapper.optimize_map(window, prune=True, iters=1)
    if first is not None and last is not None:
        s.map_loss.append((first, last))
    s.stats["map_iters"] += mapper.nr_iters - it0
    s.stats["renders"] += (mapper.nr_iters - it0) * len(window)
    s.window_sizes.append(len(window))


def _track_frame(s, vp, prev, max_iters, graph=True, exclusive=False, lookahead=1, tracker="adam"):
    """Tracks ``vp`` from the pose of ``prev`` and clears the map's grads; of ``s`` it needs ``intr``, ``bg``, ``gmap``, ``tgraph`` and
    ``stats``.  ``graph``: one captured iteration per map version (``exclusive``: only a caller that owns the box may vouch for it),
    the convergence flag read ``lookahead`` replays late, the capture accounted apart where ``stats`` has ``track_capture_s``.
    ``tracker``: "adam" (the reference's) or "gauss_newton" (``gn_tracking``), eager or captured alike."""
    stats = s.stats
    gn = tracker == "gauss_newton"
    vp.update_RT(prev.R.clone(), prev.T.clone())     # the fused pose step updates R, T in place
    with _timed(stats, "track_s") as t0:
        if graph:
            if s.tgraph is None:                       # the map changed (or first frame): capture against the new map
                s.tgraph = (GaussNewtonGraph if gn else TrackingGraph)(vp, s.intr, s.gmap, s.bg, exclusive=exclusive)
                if "track_capture_s" in stats:
                    stats["track_capture_s"] += _clock() - t0
            n_it = s.tgraph.track(vp, max_iters, lookahead=lookahead)
        else:
            n_it = (track_gauss_newton if gn else track_eager)(vp, s.intr, s.gmap, s.bg, max_iters)
    stats["track_iters"] += n_it
    stats["tracked"] += 1
    for p in s.gmap.params():
        p.grad = None
    return n_it


def _drop_tracking_graph(s):
    if s.tgraph is not None:
        s.tgraph.close()
        s.tgraph = None


def _select_keyframe(s, i, vp):
    """``(pkg, t0)`` if frame ``i`` is a keyframe -- its render against the map as it is and the OPENING time of the ``map_s`` bracket,
    which ``_map_keyframe`` closes -- else ``(None, None)``.  "interval": every ``kf_interval``-th frame; "overlap": the tracker's
    ``add_to_window`` through ``KeyframeWindow``.  ``kf_trace``: a list that gets CPU copies of each decision's inputs (tests)."""
    kfw, kf_trace = s.kfw, s.c.kf_trace
    if kfw is None and i % s.c.kf_interval != 0:
        return None, None
    t0 = _clock()
    pkg = _render_frozen(vp, s.intr, s.gmap, s.bg)
    if kfw is None:
        return pkg, t0
    from .keyframe_window import unpack_visibility
    if kf_trace is not None:
        P = int(pkg["n_touched"].numel())
        snap = dict(frame=i, window_before=list(kfw.cur_kf_list), is_window_full=kfw.is_window_full,
                    n_touched=pkg["n_touched"].cpu(), depth=pkg["depth"].cpu(), opacity=pkg["opacity"].cpu(),
                    visibility={k: unpack_visibility(kfw.visibility[k], P).cpu() for k in kfw.cur_kf_list},
                    poses={k: (v.R.detach().cpu().clone(), v.T.detach().cpu().clone())
                           for k, v in [(i, vp)] + [(k, kfw.viewpoints[k]) for k in kfw.cur_kf_list]})
    dec = kfw.observe(vp.frame_idx, vp, pkg)
    if kf_trace is not None:
        kf_trace.append(dict(snap, decision=dec, record=kfw.last_record, window_after=list(kfw.cur_kf_list)))
    if not dec.create_kf:
        return None, None
    s.stats_kf["keyframes_selected"] += 1
    s.stats_kf["evicted_by_cutoff"] += int(kfw.last_record.removed_by_cutoff >= 0)
    s.stats_kf["evicted_by_size"] += int(kfw.last_record.removed_by_size >= 0)
    return pkg, t0


def _depth_hypothesis(s, i, vp, pkg):
    """``dict(depth=...)`` for ``extend_from_frame`` of a monocular keyframe (empty for a depth sensor); the statistics stay on the
    device until ``_report``."""
    if s.c.sensor != "monocular":
        return {}
    g = torch.Generator(device=vp.rgb.device).manual_seed(2000 + int(i))
    pd, stats = pseudo_depth(None if pkg is None else pkg["depth"], None if pkg is None else pkg["opacity"], valid_rgb(vp.rgb),
                             generator=g)
    s.pseudo_depth_stats.append((i, stats))
    return dict(depth=pd)


def _map_keyframe(s, i, vp, pkg=None, t0=None):
    """As ``Mapper.run`` does per keyframe: extend the map, apply the window policy (overlap: the window as ``KeyframeWindow`` left
    it, most recent first as the reference hands it over), ``_map_window``.  CLOSES the ``map_s`` bracket ``_select_keyframe``
    opened at ``t0``.  Frame 0 comes without ``pkg`` and ``t0``: it initialises the map inside a bracket of its own.
    A monocular keyframe is extended from ``monocular.pseudo_depth``: frame 0 from the init rule, a later one from its frozen render
    ``pkg``; the noise generator is seeded from the frame index."""
    init, kfw = pkg is None, s.kfw
    with _timed(s.stats, "map_s", t0):
        if init:
            s.gmap.extend_from_frame(vp, s.intr, init=True, **_depth_hypothesis(s, i, vp, None), **s.c.extend_kw(True))
        else:
            with _timed(s.stats, "kf_extend_s"):
                s.gmap.extend_from_frame(vp, s.intr, render_opacity=pkg["opacity"], render_depth=pkg["depth"],
                                         **_depth_hypothesis(s, i, vp, pkg), **s.c.extend_kw(False))
        if kfw is None or init:
            _slide_window(s.window, vp, s.c.window_size)
        else:
            s.window[:] = [kfw.viewpoints[k] for k in kfw.cur_kf_list]
        _map_window(s, s.c.init_itr_num if init else s.c.mapping_itr_num, init=init)
        if kfw is not None:
            if init:
                kfw.bootstrap(vp.frame_idx, vp)
            rows = s.mapper.packed_visibility()       # the window's visibility rows, packed as the statistics launch left them
            if rows is None:                          # map surgery changed the map since: the mapper's (pruned) bool rows
                rows = s.mapper.occ_aware_visibility
            for k, r in rows.items():
                if k in kfw.cur_kf_list:
                    kfw.set_visibility(k, r)
    s.stats["keyframes"] += 1
    s.kf_list.append(i)
    s.size_trace.append((i, len(s.gmap)))
    _drop_tracking_graph(s)                      # the map changed: the captured tracking graph is stale


def _learn_objects(s):
    """``learn_objects``: that many ``ObjectLayerTrainer`` steps over the window, after the mapping call that just ended and
    outside every time bracket (the rates of ``_report`` stay those of tracking and mapping)."""
    if not s.c.learn_objects:
        return
    if s.obj_trainer is None:
        from .object_layer import ObjectLayerTrainer
        s.obj_trainer = ObjectLayerTrainer(s.gmap, s.intr, s.bg)
    s.obj_loss.append(s.obj_trainer.run(s.window, int(s.c.learn_objects)))


def _viewer_frames(s, vp, tag):
    """``viewer_dir``: one PNG per mode of ``viewer_modes`` from a camera behind ``vp``'s pose (the reference's ``view_dir_behind``,
    what its viewer follows the tracker with), ``<tag>_<mode>.png``: the map as it is, the keyframes' frustums and trajectory, the
    current and the ground-truth camera.  Outside every time bracket; the capacity hint of the map's shape is put back afterwards
    (an exact forward from another camera would overwrite the one the captured iterations were sized with)."""
    import os

    from . import rasterizer as R
    from .viewer import HeadlessViewer, Snapshot, save_png, view_behind
    c = s.c
    if s.viewer is None:
        os.makedirs(c.viewer_dir, exist_ok=True)
        s.viewer = HeadlessViewer(s.intr, s.bg)
    key = (len(s.gmap), int(s.intr.width), int(s.intr.height))
    hint = R.capacity_hint(*key)
    snap = Snapshot.from_map(s.gmap, [s.frames[k] for k in s.kf_list], current=vp, gt=vp if vp.R_gt is not None else None)
    cam = view_behind(vp, s.intr)
    with R.exact_counts():
        for mode in c.viewer_modes:
            path = os.path.join(c.viewer_dir, f"{tag}_{mode}.png")
            save_png(s.viewer.frame(snap, cam, mode=mode), path)
            s.viewer_files.append(path)
    if hint is None:
        R.forget_capacity(*key)
    else:
        R.reserve_capacity(*key, hint)


def _finish(s):
    """What follows the last frame; returns the result keys it adds.  ``eval_render``: ``eval`` (``evaluation.eval_rendering`` before
    and after the refinement) and ``ate`` over the keyframes, as the reference reports them.  ``refine_iters``: that many iterations
    of ``refinement.Refiner`` over all keyframes (``refinement``).  ``eager_probe``: that many iterations of
    ``eager_probe.eager_tracking_probe`` against the final map (``eager_tracking``).  ``learn_objects``: ``objects`` = the trainer's
    iteration count, its first and last loss and ``object_layer.eval_segmentation`` over the run's frames.  ``mesh_path``: ``mesh`` =
    the final map fused from every keyframe into a TSDF volume of ``mesh_voxel`` metres over the map's bounds and written there as a
    triangle-mesh PLY (``tsdf.mesh_from_map``): ``path, vertices, triangles, voxel, integrate_ms, extract_ms`` and, on the synthetic
    room, ``accuracy_mean_m`` (mean distance of the vertices to the room's true surfaces).  ``mesh_gt`` (a mesh PLY in the sequence's
    world frame, or ``"room"`` for ``sequences.room_mesh``): ``mesh["reconstruction"]`` = ``mesh_eval.eval_reconstruction`` of the written
    mesh against it, ``mesh_samples`` samples each, both culled by the keyframes (their estimated poses) and their depth images.
    ``mesh_depth_l1`` (with both): ``mesh["depth_l1"]`` = ``mesh_render.eval_depth_l1`` of the two meshes over the keyframes; a monocular
    run then culls by the rendered ground-truth mesh (``depths="render"``) instead of without an occlusion test.
    ``mesh_depth="median"`` fuses ``surface.surface_depth``'s median depth instead of the blended mean, gated by the spread
    ``mesh_max_std`` (metres; 0: no gate); the entry then also holds ``depth_mode`` and ``max_std``.  ``eval_geometry`` (with ``mesh_gt``):
    ``mesh["geometry"]`` = ``surface.eval_geometry`` of the map over the keyframes against the ground-truth mesh."""
    c, frames, gmap, intr, bg, mapper, kf_list = s.c, s.frames, s.gmap, s.intr, s.bg, s.mapper, s.kf_list
    _drop_tracking_graph(s)
    extra = {}
    if c.eval_render or c.refine_iters:
        from .evaluation import eval_ate, eval_rendering
        from .refinement import Refiner
        mapper._drop_plan()             # (its captured graphs and their overflow flags go before the refinement captures its own)
        for p in gmap.params():
            p.grad = None
        if c.eval_render:
            extra["eval"] = dict(before_opt=eval_rendering(frames, gmap, intr, bg, kf_list, tag="before_opt"))
        if c.refine_iters:
            refiner = Refiner(gmap, intr, bg, use_graph=c.graph_mapping)
            t0 = _clock()
            res = refiner.refine([frames[k] for k in kf_list], iters=int(c.refine_iters))
            res["it_per_s"] = int(c.refine_iters) / max(_clock() - t0, 1e-9)
            refiner.close()
            extra["refinement"] = res
        if c.eval_render:
            extra["eval"]["final"] = (eval_rendering(frames, gmap, intr, bg, kf_list, tag="final") if c.refine_iters
                                      else extra["eval"]["before_opt"])
            extra["ate"] = eval_ate(frames, kf_ids=kf_list)
    if c.learn_objects:
        from .object_layer import eval_segmentation
        extra["objects"] = dict(iters=s.obj_trainer.steps if s.obj_trainer is not None else 0,
                                loss_first=s.obj_loss[0][0] if s.obj_loss else None,
                                loss_last=s.obj_loss[-1][1] if s.obj_loss else None,
                                **eval_segmentation(frames, gmap, intr, bg, kf_list))
    if c.eager_probe:
        # (the captured graphs of the run and their private pools go first: the probe measures an eager caller, not one that
        #  shares its process with a few dozen instantiated hipGraphs)
        from .eager_probe import eager_tracking_probe
        mapper._drop_plan()
        mapper._pool = None
        gc.collect()
        torch.cuda.empty_cache()
        extra["eager_tracking"] = eager_tracking_probe(frames, intr, gmap, bg, int(c.eager_probe))
    if c.mesh_path is not None:          # (only then: tests/golden/run_slam_contract.json pins the keys of the default flags)
        from .tsdf import mesh_from_map
        m = mesh_from_map(gmap, [frames[k] for k in kf_list], intr, bg, float(c.mesh_voxel), path=c.mesh_path,
                          depth=c.mesh_depth, max_std=float(c.mesh_max_std))
        mesh = m.pop("mesh")
        if c.mesh_depth != "mean":       # (the default keeps exactly the keys it always had)
            m.update(depth_mode=c.mesh_depth, max_std=float(c.mesh_max_std))
        if c.sequence is None and c.scene == "room" and m["vertices"]:
            from .sequences import room_surface_distance
            m["accuracy_mean_m"] = float(room_surface_distance(mesh.vertices).mean())
        if c.mesh_gt is not None:        # (only then: the `mesh` entry of a run without it keeps exactly its keys)
            from .mesh_eval import eval_reconstruction
            if c.mesh_gt == "room":
                from .sequences import room_mesh
                gt = room_mesh(gmap._xyz.device)
            else:
                from .ply_io import load_mesh_ply
                gt = load_mesh_ply(str(c.mesh_gt), device=gmap._xyz.device)
            kfs = [frames[k] for k in kf_list]
            depths = [f.depth for f in kfs] if c.sensor == "depth" else None     # (a monocular frame's depth is the all-zero image)
            if depths is None and c.mesh_depth_l1:          # (only with the flag: an existing monocular run's figures stay)
                depths = "render"
            m["reconstruction"] = eval_reconstruction(mesh, gt, n_samples=int(c.mesh_samples), viewpoints=kfs, intr=intr, depths=depths)
            if c.mesh_depth_l1:
                from .mesh_render import eval_depth_l1
                m["depth_l1"] = eval_depth_l1(mesh, gt, kfs, intr)
            if c.eval_geometry:
                from .surface import eval_geometry
                m["geometry"] = eval_geometry(gmap, kfs, intr, bg, gt_mesh=gt)
        extra["mesh"] = m
    return extra


def _report(s, extra):
    """The result dict; with ``nr_objects`` it also holds ``map``, ``frame_list`` and ``intr``, for a caller that renders from the map."""
    c, stats, gmap, frames, ms, sl = s.c, s.stats, s.gmap, s.frames, s.mapper.stats, s.gmap.surgery_log
    err = torch.stack([position_error(f) for f in frames[1:]])
    out = dict(stats, **extra)
    if s.kfw is not None:
        out.update(s.stats_kf, kf_selection=c.kf_selection, check_viewpoints_overlap=bool(c.check_viewpoints_overlap),
                   final_window=list(s.kfw.cur_kf_list))
    out["surgery"] = dict(
        densify_and_prune_calls=len(sl), cloned=sum(e["cloned"] for e in sl), split_net=sum(e["split_net"] for e in sl),
        pruned=sum(e["pruned"] for e in sl), calls_that_grew=sum(1 for e in sl if e["cloned"] + e["split_net"] > 0),
        calls_that_pruned=sum(1 for e in sl if e["pruned"] > 0), covisibility_prunes=len(s.mapper.coviz_log),
        covisibility_pruned=sum(n for _, n in s.mapper.coviz_log),
        gaussians_after_keyframe=[n for _, n in s.size_trace], log=sl[:6] + sl[-4:] if len(sl) > 10 else sl)
    if c.nr_objects is not None:
        out.update(map=gmap, frame_list=frames, intr=s.intr)
    if c.viewer_dir is not None:         # (only then: tests/golden/run_slam_contract.json pins the keys of the default flags)
        out["viewer"] = dict(dir=str(c.viewer_dir), modes=list(c.viewer_modes), every=int(c.viewer_every), files=list(s.viewer_files))
    if c.tracker != "adam":              # (the default tracker keeps exactly the keys it always had)
        out["tracker"] = c.tracker
    if c.sensor == "monocular":          # (a depth run keeps exactly the keys it always had)
        from .evaluation import eval_ate
        out.update(sensor="monocular", ate_sim3=eval_ate(frames, align=True, correct_scale=True),
                   pseudo_depth_stats=[dict(frame=i, median=m, std=sd, count=int(n), used_init_rule=bool(r))
                                       for i, (m, sd, n, r) in ((i, st.tolist()) for i, st in s.pseudo_depth_stats)])
    out.update(frames=len(frames), gaussians=int(gmap.get_xyz.shape[0]), width=s.intr.width, height=s.intr.height,
               tracking_fps=stats["tracked"] / max(stats["track_s"], 1e-9),
               tracking_iters_per_s=stats["track_iters"] / max(stats["track_s"], 1e-9),
               mapping_iters_per_s=stats["map_iters"] / max(stats["map_s"], 1e-9),
               mapping_kf_per_s=stats["keyframes"] / max(stats["map_s"], 1e-9),
               # steady state: graph replays only (no capture, no keyframe insertion, no one-time lazy loading)
               tracking_steady_iters_per_s=(stats["track_iters"] / max(stats["track_s"] - stats["track_capture_s"], 1e-9)
                                            if c.graph_tracking else None),
               mapping_steady_iters_per_s=(ms["replays"] / max(ms.get("replay_s", 0.0), 1e-9) if ms["replays"] else None),
               mapping_keyframe_iters_per_s=(ms.get("replay_kf", 0) / max(ms.get("replay_s", 0.0), 1e-9) if ms["replays"] else None),
               mapping_replays=ms["replays"], mapping_eager_iters=ms["eager_iters"], mapping_captures=ms["captures"],
               mapping_capture_s=ms["capture_s"], window_sizes=s.window_sizes,
               kf_extend_ms=1e3 * stats["kf_extend_s"] / max(stats["keyframes"] - 1, 1),
               ate_rmse_m=float(torch.sqrt((err ** 2).mean())), position_error_m=[float(e) for e in err],
               track_iters_per_frame=s.per_frame,
               poses=[(f.R.detach().cpu().clone(), f.T.detach().cpu().clone()) for f in frames],
               camera_centers=[(-(f.R.t() @ f.T)).cpu() for f in frames],
               camera_centers_gt=[(-(f.R_gt.t() @ f.T_gt)).cpu() for f in frames],
               map_loss=[(float(a), float(b)) for a, b in s.map_loss],
               graph_tracking=bool(c.graph_tracking), graph_mapping=bool(c.graph_mapping), map_surgery=bool(c.map_surgery),
               config=dict(tracking_itr_num=c.tracking_itr_num, mapping_itr_num=c.mapping_itr_num,
                           window_size=c.window_size, kf_interval=c.kf_interval, init_itr_num=c.init_itr_num))
    return out


def run_slam(n_frames=12, intrinsics="fr3_office", tracking_itr_num=100, mapping_itr_num=150, window_size=8,
             kf_interval=4, init_itr_num=300, n_gaussians=60000, device="cuda:0", log=None,
             init_downsample=8, kf_downsample=16, point_size=1.0, graph_tracking=False, graph_mapping=False,
             track_lookahead=1, map_surgery=False, reference_lrs=False, prune_after_mapping=None,
             scene="cloud", reference_densify=False, eager_probe=0, exclusive_device=False,
             kf_selection="interval", check_viewpoints_overlap=False, kf_trace=None, refine_iters=0, eval_render=False,
             sequence=None, nr_objects=None, sensor="depth", viewer_dir=None, viewer_modes=("rgb",), viewer_every=0,
             learn_objects=0, mesh_path=None, mesh_voxel=0.02, mesh_gt=None, mesh_samples=200_000,
             mesh_depth_l1=False, tracker="adam", mesh_depth="mean", mesh_max_std=0.0, eval_geometry=False):
    """Tracks and maps a sequence in one process; returns tracking / mapping rates, iterations and the trajectory error (``_report``).
    Every argument is described where it acts: ``_setup``, ``_track_frame``, ``_select_keyframe``, ``_map_keyframe``, ``_map_window``,
    ``_finish`` (what follows the last frame).  ``log``: a callable that gets a line per frame.  ``sensor="monocular"`` adds the result
    keys ``sensor``, ``ate_sim3`` (Sim(3)-aligned ATE over all frames) and ``pseudo_depth_stats``; ``run_slam_two_process`` stays RGB-D.
    ``viewer_dir``: write headless-viewer frames there (``monogs_amd.viewer``), one per mode of ``viewer_modes``, after every
    ``viewer_every``-th keyframe (0: never) and at the end; only then does the result hold a ``viewer`` entry.
    ``learn_objects=N`` (with ``nr_objects``): learn the object rows, N trainer iterations over the window after each mapping call; only
    then does the result hold an ``objects`` entry (iterations, first and last label loss, label accuracy and mIoU).
    ``mesh_path``: write the final map's triangle mesh there (``_finish``); only then does the result hold a ``mesh`` entry;
    with ``mesh_gt`` that entry gains ``reconstruction`` and, with ``mesh_depth_l1``, ``depth_l1`` (``_finish``); ``mesh_depth``,
    ``mesh_max_std``, ``eval_geometry``: the depth that is fused and the map's geometry figures (``_finish``).
    ``tracker="gauss_newton"``: the second-order tracker of ``gn_tracking`` instead of Adam; only then does the result hold a ``tracker`` entry."""
    s = _setup(SimpleNamespace(**locals()))              # (every argument, by name: must stay the first statement)
    for i, vp in enumerate(s.frames):
        if i == 0:
            vp.update_RT(vp.R_gt, vp.T_gt)
            _map_keyframe(s, 0, vp)
            _learn_objects(s)
            if viewer_dir is not None and viewer_every > 0 and s.stats["keyframes"] % viewer_every == 0:
                _viewer_frames(s, vp, f"kf{s.stats['keyframes']:04d}")
            continue
        n_it = _track_frame(s, vp, s.frames[i - 1], tracking_itr_num, graph_tracking, exclusive_device, track_lookahead, tracker)
        s.stats["renders"] += n_it
        s.per_frame.append((i, n_it))
        pkg, t0 = _select_keyframe(s, i, vp)
        if pkg is not None:
            _map_keyframe(s, i, vp, pkg, t0)
            _learn_objects(s)
            if viewer_dir is not None and viewer_every > 0 and s.stats["keyframes"] % viewer_every == 0:
                _viewer_frames(s, vp, f"kf{s.stats['keyframes']:04d}")
        if log:
            cov = (_render_frozen(vp, s.intr, s.gmap, s.bg)["opacity"] > 0.99).float().mean().item()
            log(f"frame {i}: P={s.gmap.get_xyz.shape[0]} track_iters={s.stats['track_iters']} kf={s.stats['keyframes']} "
                f"pos_err={position_error(vp).item():.4f} m  opaque>0.99={cov:.2f}")
    extra = _finish(s)
    if viewer_dir is not None:
        _viewer_frames(s, s.frames[-1], "final")
    return _report(s, extra)


# ---- the two-process topology of the reference (/root/reference/slam.py:102-179): tracker here, mapper in a spawned process;
# the map crosses on every keyframe -- there pickled through an mp.Queue (utils/slam_mapper.py:550-564), here through `MapArena`
ARENA_FIELDS = {"xyz": (3,), "rotation": (4,), "scaling": (1,), "opacity": (1,), "rgb": (3,)}


class _ArenaMapView:       # what the tracker needs of a map, over the views a `MapArena.acquire()` hands out (already activated)
    def __init__(self, views):
        self.get_xyz, self.get_rotation, self.get_scaling = views["xyz"], views["rotation"], views["scaling"]
        self.get_opacity, self.get_features = views["opacity"], views["rgb"]

    def params(self):                     # a snapshot takes no gradient
        return ()


def _mapper_process(arena, q_in, q_out, cfg):
    """`Mapper.run` in miniature (/root/reference/utils/slam_mapper.py:566-734): wait for `init` / `keyframe` / `stop`,
    extend the map from the keyframe, optimise the window, publish the map."""
    import multiprocessing
    dev = cfg["device"]
    torch.cuda.set_device(torch.device(dev))
    frames, intr = make_sequence(cfg["n_frames"], cfg["intrinsics"], cfg["n_gaussians"], device=dev)
    bg = torch.zeros(3, device=dev)
    gmap = GaussianMap(dev)
    mapper = WindowMapper(gmap, intr, bg, window_size=cfg["window_size"], use_graph=cfg["graph"])
    mapper.map_surgery = False
    window: List[Viewpoint] = []
    try:
        while True:
            msg = q_in.get()
            if msg[0] == "stop":
                break
            tag, idx, R, T = msg
            vp = frames[idx]
            vp.update_RT(torch.tensor(R, device=dev), torch.tensor(T, device=dev))
            t0 = time.perf_counter()
            if tag == "init":
                gmap.extend_from_frame(vp, intr, downsample=cfg["init_downsample"], init=True, point_size=1.0)
                window.append(vp)
                mapper.initialize_map(vp, iters=cfg["init_itr_num"])
            else:
                pkg = _render_frozen(vp, intr, gmap, bg)
                # (unlike `_map_keyframe`: no rendered depth, so new points are tested against the frame's own depth)
                gmap.extend_from_frame(vp, intr, downsample=cfg["kf_downsample"], render_opacity=pkg["opacity"], point_size=1.0)
                _slide_window(window, vp, cfg["window_size"])
                mapper.new_keyframe_optimizers(window)
                mapper.optimize_map(window, iters=cfg["mapping_itr_num"])      # (one call: nobody records the first loss here)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            with torch.no_grad():
                seq = arena.publish({"xyz": gmap.get_xyz, "rotation": gmap.get_rotation, "scaling": gmap.get_scaling,
                                     "opacity": gmap.get_opacity, "rgb": gmap.get_features})
            t2 = time.perf_counter()
            # (the keyframe's refined pose goes back with the answer, as `sync_backend` carries the keyframes back)
            q_out.put(("done", idx, seq, len(gmap), t1 - t0, t2 - t1, vp.R.cpu().numpy(), vp.T.cpu().numpy(), len(window)))
    finally:
        multiprocessing.current_process()._args = ()       # (a spawned child leaves through os._exit: drop the IPC mappings now)
        del arena
        gc.collect()
        torch.cuda.ipc_collect()


def run_slam_two_process(n_frames=12, intrinsics="fr3_office", tracking_itr_num=100, mapping_itr_num=150, window_size=8,
                         kf_interval=4, init_itr_num=150, n_gaussians=60000, device="cuda:0", capacity=400000, graph=True,
                         init_downsample=8, kf_downsample=16):
    """The tracking / mapping loops of `run_slam` split over two processes as the reference runs them, with the map handed
    over through `MapArena`.  The tracker (this process) tracks every frame against the
    snapshot it last acquired and, on a keyframe, asks the mapper and waits for the next publish -- the reference's
    tracker does the same (`utils/slam_tracker.py:362-365`).  Returns rates, the hand-off times and the trajectory error."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    arena = MapArena(capacity, ARENA_FIELDS, device=device)
    q_in, q_out = ctx.Queue(), ctx.Queue()
    cfg = dict(n_frames=n_frames, intrinsics=intrinsics, n_gaussians=n_gaussians, device=device, window_size=window_size,
               init_itr_num=init_itr_num, mapping_itr_num=mapping_itr_num, graph=graph, init_downsample=init_downsample,
               kf_downsample=kf_downsample)
    proc = ctx.Process(target=_mapper_process, args=(arena, q_in, q_out, cfg))
    proc.start()
    frames, intr = make_sequence(n_frames, intrinsics, n_gaussians, device=device)
    bg = torch.zeros(3, device=device)
    stats = dict(track_s=0.0, track_iters=0, tracked=0, wait_s=0.0, acquire_s=0.0, publish_s=0.0, map_s=0.0, keyframes=0)
    windows, sizes, seqs, seq = [], [], [], 0
    s = SimpleNamespace(intr=intr, bg=bg, gmap=None, tgraph=None, stats=stats)      # for `_track_frame`; `gmap`: the last snapshot
    t_all = time.perf_counter()

    def ask(tag, vp):
        nonlocal seq
        t0 = time.perf_counter()
        q_in.put((tag, vp.frame_idx, vp.R.cpu().numpy(), vp.T.cpu().numpy()))
        deadline = time.perf_counter() + 600.0
        while True:                       # a dead mapper must not leave the tracker blocked for ten minutes
            try:
                ans = q_out.get(timeout=1.0)
                break
            except queue.Empty:
                if not proc.is_alive():
                    raise RuntimeError(f"the mapper process died (exit code {proc.exitcode}) while the tracker waited for keyframe "
                                       f"{vp.frame_idx}") from None
                if time.perf_counter() > deadline:
                    raise RuntimeError("the mapper process did not answer within 600 s") from None
        stats["wait_s"] += time.perf_counter() - t0
        _, idx, new_seq, P, t_map, t_pub, R, T, wlen = ans
        stats["map_s"] += t_map
        stats["publish_s"] += t_pub
        stats["keyframes"] += 1
        t1 = time.perf_counter()
        got, views = arena.acquire()
        stats["acquire_s"] += time.perf_counter() - t1
        assert got == new_seq and int(views["xyz"].shape[0]) == P, (got, new_seq, P)
        vp.update_RT(torch.tensor(R, device=device), torch.tensor(T, device=device))
        _drop_tracking_graph(s)
        s.gmap, seq = _ArenaMapView(views), got
        windows.append(wlen); sizes.append(P); seqs.append(got)
    try:
        for i, vp in enumerate(frames):
            if i == 0:
                vp.update_RT(vp.R_gt, vp.T_gt)
                ask("init", vp)
                continue
            _track_frame(s, vp, frames[i - 1], tracking_itr_num)      # (not exclusive: the mapper process shares the device)
            assert not arena.stale(seq), "the mapper overwrote the snapshot the tracker was reading"
            if i % kf_interval == 0:
                ask("keyframe", vp)
    finally:
        _drop_tracking_graph(s)
        q_in.put(("stop",))
        proc.join(timeout=120)
        if proc.is_alive():               # hung: do not leave a child holding a HIP context and the IPC mappings behind
            proc.terminate()
            proc.join(timeout=10)
            if proc.is_alive():
                proc.kill()
                proc.join(timeout=10)
        s.gmap = None
        del arena
        for _ in range(5):
            gc.collect()
            torch.cuda.ipc_collect()
            time.sleep(0.05)
    wall = time.perf_counter() - t_all
    exitcode = proc.exitcode
    if exitcode != 0:
        raise RuntimeError(f"the mapper process ended with exit code {exitcode}")
    err = torch.stack([position_error(f) for f in frames[1:]])
    k = max(stats["keyframes"], 1)
    return dict(stats, frames=n_frames, wall_s=wall, fps_end_to_end=(n_frames - 1) / wall,
                tracking_iters_per_s=stats["track_iters"] / max(stats["track_s"], 1e-9),
                tracking_fps=stats["tracked"] / max(stats["track_s"], 1e-9),
                handoff_ms=dict(publish=1e3 * stats["publish_s"] / k, acquire=1e3 * stats["acquire_s"] / k),
                mapper_busy_ms_per_keyframe=1e3 * stats["map_s"] / k, window_sizes=windows, gaussians=sizes, sequences=seqs,
                ate_rmse_m=float(torch.sqrt((err ** 2).mean())), exitcode=exitcode)
