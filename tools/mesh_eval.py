#!/usr/bin/env python3
"""Score a reconstructed mesh against a ground-truth mesh (monogs_amd.mesh_eval): accuracy, completion, completion ratio,
Chamfer-L1 and precision / recall / F-score between area-weighted samples of both.  Both files are binary little-endian PLY meshes
in the same world frame (what ``save_mesh_ply`` writes; Replica's ``mesh.ply`` with its quads and uint indices).  No visibility cull
here: that needs the cameras (``run_slam(mesh_gt=...)`` / ``tools/slam_bench.py --mesh-gt``).  Prints the dictionary as one JSON line.

    python tools/mesh_eval.py REC.ply GT.ply [--samples 200000] [--threshold 0.05] [--seed 0]
    python tools/mesh_eval.py REC.ply GT.ply --depth-l1 --poses FILE [--width 1200 --height 680 --fx 600 --fy 600 --cx 599.5 --cy 339.5]
        # adds `depth_l1` (monogs_amd.mesh_render.eval_depth_l1): both meshes rendered from every pose of FILE, one pose per line as
        # 12 numbers, the rows of the 3 x 4 world->camera matrix [R | t]; `#` starts a comment"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_poses(text: str):
    """``[(R, t)]`` (nested lists: 3 x 3 and 3) from one pose per line as 12 world->camera numbers, the rows of ``[R | t]``.  Blank lines
    and ``#`` comments are skipped; any other line that does not hold exactly 12 finite numbers is refused with its line number."""
    import math
    poses = []
    for n, line in enumerate(text.splitlines(), 1):
        body = line.split("#", 1)[0].strip()
        if not body:
            continue
        fields = body.replace(",", " ").split()
        try:
            x = [float(f) for f in fields]
        except ValueError:
            raise ValueError(f"pose file line {n}: not a number in {body!r}") from None
        if len(x) != 12 or not all(math.isfinite(v) for v in x):
            raise ValueError(f"pose file line {n}: expected 12 finite numbers (the rows of the 3 x 4 world->camera matrix), got {len(x)}")
        poses.append(([x[0:3], x[4:7], x[8:11]], [x[3], x[7], x[11]]))
    return poses


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rec", metavar="REC.ply")
    ap.add_argument("gt", metavar="GT.ply")
    ap.add_argument("--samples", type=int, default=200000, help="samples per mesh")
    ap.add_argument("--threshold", type=float, default=0.05, help="metres: completion ratio, precision, recall")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--depth-l1", action="store_true", help="also Depth L1 between the two meshes rendered from --poses")
    ap.add_argument("--poses", default=None, metavar="FILE", help="one world->camera pose per line, 12 numbers")
    ap.add_argument("--max-depth", type=float, default=0.0, help="with --depth-l1: ignore pixels beyond this depth (0: none)")
    for name, default in (("width", 1200), ("height", 680)):
        ap.add_argument(f"--{name}", type=int, default=default)
    for name, default in (("fx", 600.0), ("fy", 600.0), ("cx", 599.5), ("cy", 339.5)):
        ap.add_argument(f"--{name}", type=float, default=default)
    a = ap.parse_args()
    if a.depth_l1 != (a.poses is not None):
        ap.error("--depth-l1 and --poses go together")
    poses = None
    if a.poses is not None:
        with open(a.poses) as f:
            try:
                poses = parse_poses(f.read())
            except ValueError as e:
                ap.error(f"{a.poses}: {e}")
        if not poses:
            ap.error(f"{a.poses} holds no pose")
    from monogs_amd.mesh_eval import eval_reconstruction
    from monogs_amd.ply_io import load_mesh_ply
    rec, gt = load_mesh_ply(a.rec, device="cuda:0"), load_mesh_ply(a.gt, device="cuda:0")
    out = eval_reconstruction(rec, gt, n_samples=a.samples, threshold=a.threshold, seed=a.seed)
    if poses is not None:
        import torch
        from monogs_amd.frames import Intrinsics
        from monogs_amd.mesh_render import eval_depth_l1
        intr = Intrinsics(dict(fx=a.fx, fy=a.fy, cx=a.cx, cy=a.cy, W=a.width, H=a.height), "cuda:0")
        views = [(torch.tensor(R, dtype=torch.float32, device="cuda:0"), torch.tensor(t, dtype=torch.float32, device="cuda:0")) for R, t in poses]
        out["depth_l1"] = eval_depth_l1(rec, gt, views, intr, max_depth=a.max_depth)
    out.update(rec=a.rec, gt=a.gt, rec_triangles=int(rec.triangles.shape[0]), gt_triangles=int(gt.triangles.shape[0]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
