#!/usr/bin/env python3
"""Score a reconstructed mesh against a ground-truth mesh (monogs_amd.mesh_eval): accuracy, completion, completion ratio,
Chamfer-L1 and precision / recall / F-score between area-weighted samples of both.  Both files are binary little-endian PLY meshes
in the same world frame (what ``save_mesh_ply`` writes; Replica's ``mesh.ply`` with its quads and uint indices).  No visibility cull
here: that needs the cameras (``run_slam(mesh_gt=...)`` / ``tools/slam_bench.py --mesh-gt``).  Prints the dictionary as one JSON line.

    python tools/mesh_eval.py REC.ply GT.ply [--samples 200000] [--threshold 0.05] [--seed 0]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rec", metavar="REC.ply")
    ap.add_argument("gt", metavar="GT.ply")
    ap.add_argument("--samples", type=int, default=200000, help="samples per mesh")
    ap.add_argument("--threshold", type=float, default=0.05, help="metres: completion ratio, precision, recall")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from monogs_amd.mesh_eval import eval_reconstruction
    from monogs_amd.ply_io import load_mesh_ply
    rec, gt = load_mesh_ply(a.rec, device="cuda:0"), load_mesh_ply(a.gt, device="cuda:0")
    out = eval_reconstruction(rec, gt, n_samples=a.samples, threshold=a.threshold, seed=a.seed)
    out.update(rec=a.rec, gt=a.gt, rec_triangles=int(rec.triangles.shape[0]), gt_triangles=int(gt.triangles.shape[0]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
