#!/usr/bin/env python3
"""Tracking + mapping FPS of the two SLAM hot loops on a synthetic sequence (BASELINE configs 3-4
stand-in; the TUM / Replica sequences are not available offline).  Prints one JSON line.
  python tools/slam_bench.py --config tum      # 640x480, tracking 100 / mapping 150 / window 8 / kf 5
  python tools/slam_bench.py --config replica  # 1200x680, tracking 100 / mapping 150 / window 10 / kf 4
  python tools/slam_bench.py --config tum --dataset CONFIG.yaml --frames 200 [--stride 2]
      # a TUM / Replica sequence on disk (monogs_amd.dataset), or an EuRoC stereo one (Dataset.sensor_type: stereo,
      # monogs_amd.stereo): size and intrinsics from the YAML, iteration counts from --config
  python tools/slam_bench.py --config tum --room --graph --sensor monocular
      # no depth: RGB-only losses, keyframes back-projected from depth hypotheses (monogs_amd.monocular); with --dataset the depth
      # files are not read (a YAML with Dataset.sensor_type: monocular selects this by itself).  Prints both ATEs to stderr.
  python tools/slam_bench.py --config tum --room --viewer frames/ --viewer-modes rgb depth elipsoids --viewer-every 2
      # PNGs of what the reference's viewer window would show, from a camera behind the current pose (monogs_amd.viewer)
  python tools/slam_bench.py --config tum --room --graph --mesh room.ply [--mesh-voxel 0.02]
      # the final map fused from every keyframe into a TSDF volume and written as a coloured triangle mesh (monogs_amd.tsdf)
  python tools/slam_bench.py --config tum --room --graph --mesh room.ply --mesh-gt room
      # ... and scored against the ground-truth mesh: accuracy, completion, completion ratio, Chamfer-L1, F-score (monogs_amd.mesh_eval)
  python tools/slam_bench.py --config tum --room --graph --mesh room.ply --mesh-gt room --mesh-depth-l1
      # ... and Depth L1 between the two meshes rendered from the keyframes (monogs_amd.mesh_render)
  python tools/slam_bench.py --config tum --room --graph --mesh room.ply --mesh-gt room --mesh-depth median [--mesh-max-std 0.05] --eval-geometry
      # ... fused from the median depth instead of the blended mean, and the map's depth and normals against the ground truth (monogs_amd.surface)
  python tools/slam_bench.py --config tum --room --graph --tracker gauss_newton
      # the Gauss-Newton tracker (monogs_amd.gn_tracking) instead of Adam: fewer, heavier tracking iterations per frame
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    # /root/reference/configs/mono/tum/base_config.yaml:24-33
    "tum": dict(intrinsics="fr3_office", tracking_itr_num=100, mapping_itr_num=150, window_size=8, kf_interval=5),
    # /root/reference/configs/rgbd/replica/base_config.yaml:39-48
    "replica": dict(intrinsics="replica", tracking_itr_num=100, mapping_itr_num=150, window_size=10, kf_interval=4),
}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tum", choices=list(CONFIGS))
    ap.add_argument("--frames", type=int, default=11)
    ap.add_argument("--init-iters", type=int, default=300)
    ap.add_argument("--mapping-iters", type=int, default=None)
    ap.add_argument("--tracking-iters", type=int, default=None)
    ap.add_argument("--window", type=int, default=None)
    ap.add_argument("--kf-interval", type=int, default=None)
    ap.add_argument("--gaussians", type=int, default=60000)
    ap.add_argument("--graph", action="store_true", help="replay the tracking and the mapping iteration from hipGraphs (capacity mode)")
    ap.add_argument("--eager-mapping", action="store_true", help="with --graph: capture tracking only")
    ap.add_argument("--surgery", action="store_true", help="densify_and_prune / opacity resets / covisibility pruning on the reference's schedule")
    ap.add_argument("--reference-lrs", action="store_true", help="the reference's learning rates + xyz schedule")
    ap.add_argument("--room", action="store_true", help="opaque box-room sequence (ray-cast) instead of the semi-transparent cloud")
    ap.add_argument("--reference-densify", action="store_true",
                    help="new Gaussians as the fork hard-codes them: 1/32 (init) and 1/64 of the pixels, scale^2 = dist2 x min(0.05, 0.01 x median depth)")
    ap.add_argument("--eager-probe", type=int, default=0, help="after the run: N iterations of the unmodified eager tracking loop, timed")
    ap.add_argument("--fork", action="store_true",
                    help="the values the fork hard-codes over its YAML (/root/reference/utils/slam_tracker.py:70-72, "
                         "utils/slam_mapper.py:64-89,660-662, slam.py:75): tracking 100, every frame a keyframe, init 1050, "
                         "300 iterations per keyframe, window 30")
    ap.add_argument("--lookahead", type=int, default=1, choices=[0, 1],
                    help="with --graph: read the convergence flag of tracking iteration n-1 while n runs")
    ap.add_argument("--kf-selection", default="interval", choices=["interval", "overlap"],
                    help="overlap: keyframes and evictions decided on the device (monogs_amd.keyframe_window) instead of every "
                         "--kf-interval-th frame")
    ap.add_argument("--check-overlap", action="store_true",
                    help="with --kf-selection overlap: the tracker's check_viewpoints_overlap (upstream MonoGS; False in the fork)")
    ap.add_argument("--refine", type=int, default=0, metavar="N",
                    help="after the run: N iterations of the colour refinement (Mapper.refinement runs 26000), captured with --graph")
    ap.add_argument("--eval", action="store_true",
                    help="PSNR / SSIM on every fifth non-keyframe before and after the refinement, and the ATE statistics")
    ap.add_argument("--dataset", default=None, metavar="CONFIG.yaml",
                    help="run on the TUM / Replica / EuRoC sequence this reference-style YAML names (Dataset.type, dataset_path, "
                         "Calibration) instead of a synthetic one: --frames frames from the first, every --stride-th")
    ap.add_argument("--stride", type=int, default=1, help="with --dataset: take every N-th frame")
    ap.add_argument("--sensor", default=None, choices=["depth", "monocular"],
                    help="monocular: run without depth (default: what the --dataset YAML's Dataset.sensor_type says, else depth)")
    ap.add_argument("--viewer", default=None, metavar="DIR",
                    help="write headless-viewer frames (monogs_amd.viewer) to DIR: after every --viewer-every-th keyframe and at the end")
    ap.add_argument("--viewer-modes", nargs="+", default=["rgb"], choices=["rgb", "segmentation", "depth", "time", "elipsoids"])
    ap.add_argument("--viewer-every", type=int, default=0, help="with --viewer: a frame set after every N-th keyframe (0: only at the end)")
    ap.add_argument("--learn-objects", type=int, default=0, metavar="N",
                    help="with --room: an object row per Gaussian (one score per room surface), learned from the frames' surface ids, "
                         "N trainer iterations over the window after each mapping call (monogs_amd.object_layer); the result gains "
                         "`objects`: label loss, pixel accuracy and mIoU on every fifth non-keyframe")
    ap.add_argument("--mesh", default=None, metavar="PATH",
                    help="after the run: fuse the final map from every keyframe into a TSDF volume over the map's bounds and write the "
                         "triangle mesh to PATH (binary PLY); the result gains `mesh`")
    ap.add_argument("--mesh-voxel", type=float, default=0.02, help="with --mesh: the voxel edge in metres")
    ap.add_argument("--mesh-gt", default=None, metavar="PATH|room",
                    help="with --mesh: the ground-truth mesh (a PLY in the sequence's world frame, e.g. Replica's mesh.ply; `room`: the "
                         "--room scene's true surfaces); `mesh` gains `reconstruction`: accuracy, completion, completion ratio, Chamfer-L1, "
                         "precision / recall / F-score between samples of both meshes, culled by the keyframes (monogs_amd.mesh_eval)")
    ap.add_argument("--mesh-samples", type=int, default=200000, help="with --mesh-gt: samples per mesh")
    ap.add_argument("--mesh-depth-l1", action="store_true",
                    help="with --mesh-gt: `mesh` gains `depth_l1`, the two meshes rendered from the keyframes and compared "
                         "(monogs_amd.mesh_render.eval_depth_l1)")
    ap.add_argument("--mesh-depth", default="mean", choices=["mean", "median"],
                    help="with --mesh: the depth that is fused -- the alpha-blended mean over the opacity, or the median depth of "
                         "monogs_amd.surface (the contributor at which the transmittance falls through one half); `mesh` gains `depth_mode`")
    ap.add_argument("--mesh-max-std", type=float, default=0.0, metavar="S",
                    help="with --mesh-depth median: skip pixels whose depth along the ray spreads by more than S metres (0: no gate)")
    ap.add_argument("--eval-geometry", action="store_true",
                    help="with --mesh-gt: `mesh` gains `geometry`, the L1 of the mean and of the median depth and the angle of their "
                         "normals against the ground-truth mesh rendered from the keyframes (monogs_amd.surface.eval_geometry)")
    ap.add_argument("--tracker", default="adam", choices=["adam", "gauss_newton"],
                    help="gauss_newton: track with second-order steps on the pose-tangent planes (monogs_amd.gn_tracking) instead of "
                         "Adam; the result gains `tracker`, compare `track_iters_per_frame` and `tracking_fps`")
    a = ap.parse_args()
    if a.mesh_gt and not a.mesh:
        ap.error("--mesh-gt evaluates the mesh --mesh writes")
    if a.mesh_depth_l1 and not a.mesh_gt:
        ap.error("--mesh-depth-l1 compares the mesh with --mesh-gt")
    if a.mesh_depth != "mean" and not a.mesh:
        ap.error("--mesh-depth chooses what --mesh fuses")
    if a.mesh_max_std and a.mesh_depth != "median":
        ap.error("--mesh-max-std gates the median depth: it needs --mesh-depth median")
    if a.eval_geometry and not a.mesh_gt:
        ap.error("--eval-geometry compares the map with --mesh-gt")
    from monogs_amd.slam_harness import run_slam
    cfg = dict(CONFIGS[a.config])
    init_iters = a.init_iters
    if a.fork:
        cfg.update(tracking_itr_num=100, mapping_itr_num=300, window_size=30, kf_interval=1)
        init_iters = 1050
    for k, v in (("mapping_itr_num", a.mapping_iters), ("tracking_itr_num", a.tracking_iters), ("window_size", a.window),
                 ("kf_interval", a.kf_interval)):
        if v is not None:
            cfg[k] = v
    sequence, sensor = None, a.sensor or "depth"
    if a.dataset:
        from monogs_amd.dataset import dataset_frames, load_config, load_dataset
        config = load_config(a.dataset)
        if config["Dataset"].get("sensor_type") == "stereo":     # EuRoC: depth from semi-global matching (monogs_amd.stereo)
            from monogs_amd.stereo import load_stereo_dataset as load_dataset
        if a.sensor is None and config["Dataset"].get("sensor_type") == "monocular":
            sensor = "monocular"
        mono = dict(monocular=True, config=config) if sensor == "monocular" else {}
        sequence = dataset_frames(load_dataset(config, device="cuda:0"), a.frames, device="cuda:0", stride=a.stride, **mono)
        cfg.pop("intrinsics")                           # (the YAML's calibration is the camera)
    objects = {}
    if a.learn_objects:
        if not a.room or a.dataset:
            ap.error("--learn-objects needs the segmentation of the --room sequence")
        from monogs_amd.sequences import ROOM_SURFACES
        objects = dict(nr_objects=ROOM_SURFACES, learn_objects=a.learn_objects)
    out = run_slam(sequence=sequence, n_frames=a.frames, init_itr_num=init_iters, n_gaussians=a.gaussians, graph_tracking=a.graph,
                   graph_mapping=a.graph and not a.eager_mapping, track_lookahead=a.lookahead, map_surgery=a.surgery,
                   reference_lrs=a.reference_lrs, scene="room" if a.room else "cloud", reference_densify=a.reference_densify,
                   eager_probe=a.eager_probe, kf_selection=a.kf_selection, check_viewpoints_overlap=a.check_overlap,
                   refine_iters=a.refine, eval_render=a.eval, sensor=sensor, viewer_dir=a.viewer,
                   viewer_modes=tuple(a.viewer_modes), viewer_every=a.viewer_every, log=lambda s: print("[slam]", s, file=sys.stderr, flush=True), **objects, **cfg,
                   **(dict(mesh_path=a.mesh, mesh_voxel=a.mesh_voxel) if a.mesh else {}),
                   **(dict(mesh_gt=a.mesh_gt, mesh_samples=a.mesh_samples) if a.mesh_gt else {}),
                   **(dict(mesh_depth_l1=True) if a.mesh_depth_l1 else {}),
                   **(dict(mesh_depth=a.mesh_depth, mesh_max_std=a.mesh_max_std) if a.mesh_depth != "mean" else {}),
                   **(dict(eval_geometry=True) if a.eval_geometry else {}),
                   **(dict(tracker=a.tracker) if a.tracker != "adam" else {}))
    what = f"{a.dataset}, every {a.stride}. frame" if a.dataset else f"synthetic {a.config}-like sequence"
    out["workload"] = f"{what}, {a.frames} frames" + (" (fork's hard-coded run configuration)" if a.fork else "")
    if sensor == "monocular":
        print(f"[slam] monocular: ATE rmse {out['ate_rmse_m']:.4f} m raw, {out['ate_sim3']['rmse']:.4f} m after Sim(3) alignment "
              f"({out['ate_sim3']['n']} frames)", file=sys.stderr, flush=True)
    for k in ("poses", "camera_centers", "camera_centers_gt", "map", "frame_list", "intr"):      # tensors and objects: not JSON
        out.pop(k, None)
    print(json.dumps(out))
