#!/usr/bin/env python3
"""Render a saved map (a PLY as ``monogs_amd.ply_io.save_ply`` / the reference's ``save_ply`` write it) from an orbit of free
cameras with the headless viewer (monogs_amd.viewer): ``DIR/view_0000.png`` ...

    python tools/render_views.py MAP.ply --orbit 12 --mode elipsoids --out views/ [--width 640 --height 480 --fov 60]
        [--radius R] [--height-offset H] [--scale-modifier S]

The orbit circles the map's median centre at ``--radius`` (default: twice the median distance of the Gaussians from it), the
image's up direction being -y of the map's frame (the first camera's up in a SLAM map).  The ``segmentation`` mode needs a PLY that
carries the object rows (``save_ply(..., obj_prob=gmap._obj_prob)``): each Gaussian is painted with the palette colour of its
most probable object, as the reference's viewer does.

    python tools/render_views.py --mesh MESH.ply --orbit 12 --mode depth --out views/

draws a triangle-mesh PLY (``save_mesh_ply`` / Replica's ``mesh.ply``) with the mesh renderer (monogs_amd.mesh_render) through the
same orbit cameras, in the modes ``rgb`` (vertex colours; a mesh without them is drawn grey) and ``depth``."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def render_mesh_views(a):
    from monogs_amd import viewer as V
    from monogs_amd.frames import Intrinsics
    from monogs_amd.mesh_render import MeshRenderer
    from monogs_amd.ply_io import load_mesh_ply
    from monogs_amd.tsdf import TriangleMesh
    dev = "cuda:0"
    mesh = load_mesh_ply(a.mesh, device=dev)
    if mesh.colors is None:
        mesh = TriangleMesh(mesh.vertices, mesh.triangles, torch.full_like(mesh.vertices, 0.7))
    f = a.width / (2.0 * math.tan(math.radians(a.fov) / 2.0))
    intr = Intrinsics(dict(fx=f, fy=f, cx=a.width / 2.0, cy=a.height / 2.0, W=a.width, H=a.height), dev)
    centre = mesh.vertices.median(0).values
    radius = a.radius if a.radius is not None else 2.0 * float((mesh.vertices - centre).norm(dim=1).median())
    renderer = MeshRenderer(intr, dev)
    os.makedirs(a.out, exist_ok=True)
    for i, cam in enumerate(V.orbit(centre.cpu().numpy(), radius, a.orbit, height=a.height_offset)):
        R = torch.tensor(cam.R, dtype=torch.float32, device=dev)
        T = torch.tensor(cam.T, dtype=torch.float32, device=dev)
        out = renderer.render(mesh, R, T, want=("depth", "rgb"))
        if a.mode == "rgb":
            img = out["rgb"].clamp(0, 1).permute(1, 2, 0)
        else:                                           # near = bright; nothing hit = black
            d = out["depth"]
            far = d.max().clamp_min(1e-6)
            img = torch.where(d > 0, 1.0 - 0.9 * d / far, torch.zeros_like(d))[..., None].expand(-1, -1, 3)
        path = os.path.join(a.out, f"view_{i:04d}.png")
        V.save_png((img * 255.0).to(torch.uint8).contiguous(), path)
        print(path)
    renderer.status()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ply", nargs="?", default=None)
    ap.add_argument("--mesh", default=None, metavar="MESH.ply", help="draw this triangle mesh instead of a map (modes rgb and depth)")
    ap.add_argument("--orbit", type=int, default=8, metavar="N")
    ap.add_argument("--mode", default="rgb", choices=["rgb", "segmentation", "depth", "time", "elipsoids"])
    ap.add_argument("--out", required=True, metavar="DIR")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--fov", type=float, default=60.0, help="horizontal field of view in degrees")
    ap.add_argument("--radius", type=float, default=None)
    ap.add_argument("--height-offset", type=float, default=0.0)
    ap.add_argument("--scale-modifier", type=float, default=1.0)
    a = ap.parse_args()
    if (a.ply is None) == (a.mesh is None):
        ap.error("give a map PLY or --mesh MESH.ply")
    if a.mesh is not None and a.mode not in ("rgb", "depth"):
        ap.error("--mesh is drawn in the modes rgb and depth")
    if not torch.cuda.is_available():
        sys.exit("render_views needs a GPU: the viewer has no CPU path")
    if a.mesh is not None:
        return render_mesh_views(a)
    from monogs_amd import viewer as V
    from monogs_amd.frames import Intrinsics
    from monogs_amd.ply_io import load_ply
    dev = "cuda:0"
    m = load_ply(a.ply, device=dev)
    # the file holds raw parameters: the reference's activations (gaussian_model.py:84-106); colours are stored as they are used
    if a.mode == "segmentation" and "obj_prob" not in m:
        sys.exit(f"{a.ply} holds no obj_prob_* properties: the segmentation mode needs a map saved with its object rows")
    obj_idx = m["obj_prob"].argmax(dim=1) if "obj_prob" in m else None        # (argmax of the raw row = argmax of its softmax)
    snap = V.Snapshot(m["xyz"], torch.nn.functional.normalize(m["rotation"]), torch.exp(m["scaling"]), torch.sigmoid(m["opacity"]),
                      m["f_dc"][:, :3].contiguous(), obj_idx, (), None, None)
    f = a.width / (2.0 * math.tan(math.radians(a.fov) / 2.0))
    intr = Intrinsics(dict(fx=f, fy=f, cx=a.width / 2.0, cy=a.height / 2.0, W=a.width, H=a.height), dev)
    centre = snap.means.median(0).values
    radius = a.radius if a.radius is not None else 2.0 * float((snap.means - centre).norm(dim=1).median())
    hv = V.HeadlessViewer(intr, torch.zeros(3, device=dev))
    os.makedirs(a.out, exist_ok=True)
    for i, cam in enumerate(V.orbit(centre.cpu().numpy(), radius, a.orbit, height=a.height_offset)):
        path = os.path.join(a.out, f"view_{i:04d}.png")
        V.save_png(hv.frame(snap, cam, mode=a.mode, scale_modifier=a.scale_modifier, cameras=False, trajectory=False), path)
        print(path)


if __name__ == "__main__":
    main()
