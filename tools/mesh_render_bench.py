#!/usr/bin/env python3
"""Device time of mesh rendering (monogs_amd.mesh_render, csrc/mesh_render.hip) at 640 x 480 and 1200 x 680, camera inside the room:

  room_0.1    ``sequences.room_mesh(max_edge=0.1)``: about 70 k triangles of tens of pixels each;
  room_0.02   the same at 0.02: about 1.8 M triangles, scan density, sub-pixel to a few pixels each;
  box_12      the room's six walls as two triangles each: every triangle covers a large part of the image.

Per mesh and size: one ``MeshRenderer.render`` call (depth, id, colour) eager, replayed from a captured graph, and eager with
every triangle sent through the raster pass (``fuse_small=False``: the alternative the setup kernel's small-triangle path replaced),
and beside it
  copy        a device copy of the bytes the call must move: the triangle records once (64 bytes each), the key image written and read
              once (8 bytes a pixel each way), the outputs (depth, id, three colour planes);
  gaussians   the plain no-grad forward of the same frame on the map of a short ``run_slam(scene="room")`` at that size;
and, once per size, ``eval_depth_l1`` of the 0.1 room against itself over 8 views as host wall time (its one read-back included).

Every device figure is a pair of events around one call, after --warmup calls of each variant; variants alternate call by call and
the figure is the median of --calls calls (min and max beside it).  Prints one JSON line.  The split by kernel comes from the
profiler over the eager calls alone:

    python tools/mesh_render_bench.py [--calls 20] [--warmup 3] [--no-gaussians]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_render_bench.py --kernels room_0.02 --size 640x480"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"640x480": dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6, W=640, H=480),
         "1200x680": dict(fx=600.0, fy=600.0, cx=599.5, cy=339.5, W=1200, H=680)}
WANT = ("depth", "tri_id", "rgb")


def stats(v):
    s = sorted(v)
    return {"median_us": round(1e3 * s[len(s) // 2], 1), "min_us": round(1e3 * s[0], 1), "max_us": round(1e3 * s[-1], 1)}


def timed(variants, calls, warmup):
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(calls):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: stats(v) for k, v in ms.items()}


def meshes(dev, names):
    from monogs_amd.sequences import _ROOM_HALF, room_mesh
    from monogs_amd.tsdf import TriangleMesh
    out = {}
    if "room_0.1" in names:
        out["room_0.1"] = room_mesh(dev, 0.1, colors=True)
    if "room_0.02" in names:
        out["room_0.02"] = room_mesh(dev, 0.02, colors=True)
    if "box_12" in names:
        hx, hy, hz = _ROOM_HALF
        v = torch.tensor([[sx * hx, sy * hy, sz * hz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=torch.float32, device=dev)
        quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
        t = torch.tensor([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], dtype=torch.int32, device=dev)
        out["box_12"] = TriangleMesh(v, t, (v / torch.tensor(_ROOM_HALF, device=dev) * 0.4 + 0.5).contiguous())
    return out


def room_pose(dev, k=3):
    from monogs_amd.sequences import make_room_sequence
    frames, _ = make_room_sequence(6, dict(fx=4.0, fy=4.0, cx=2.0, cy=2.0, W=4, H=4), device="cpu", step_scale=40)
    return [(f.R_gt.to(dev).contiguous(), f.T_gt.to(dev).contiguous()) for f in frames]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-gaussians", action="store_true", help="skip the SLAM run behind the Gaussian-forward yardstick")
    ap.add_argument("--kernels", default=None, metavar="MESH", help="only --calls eager calls of this mesh at --size: for a profiler run")
    ap.add_argument("--size", default="640x480", choices=sorted(SIZES))
    ap.add_argument("--no-small", action="store_true", help="with --kernels: every triangle through the raster pass (fuse_small=False)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_render_bench needs a GPU: there is no CPU path to time")
    from monogs_amd.frames import Intrinsics
    from monogs_amd.mesh_render import MeshRenderer, eval_depth_l1
    dev = "cuda:0"
    poses = room_pose(dev)
    R, T = poses[3]
    if a.kernels:
        mesh = meshes(dev, [a.kernels])[a.kernels]
        r = MeshRenderer(Intrinsics(SIZES[a.size], dev), dev)
        for _ in range(a.calls):
            r.render(mesh, R, T, want=WANT, fuse_small=not a.no_small)
        torch.cuda.synchronize()
        print(json.dumps(dict(mesh=a.kernels, size=a.size, calls=a.calls, status=r.status())))
        return
    ms = meshes(dev, ["room_0.1", "room_0.02", "box_12"])
    out = {}
    for size, k in SIZES.items():
        intr = Intrinsics(k, dev)
        HW = k["W"] * k["H"]
        res = {}
        gauss = None
        if not a.no_gaussians:
            from monogs_amd.slam_harness import _render_frozen, run_slam
            run = run_slam(n_frames=4, intrinsics=k, tracking_itr_num=20, mapping_itr_num=20, init_itr_num=100, window_size=4, kf_interval=2,
                           scene="room", nr_objects=16)
            gmap, vp, bg = run["map"], run["frame_list"][0], torch.zeros(3, device=dev)
            res["gaussians_in_map"] = int(gmap.get_xyz.shape[0])
            gauss = lambda: _render_frozen(vp, run["intr"], gmap, bg)  # noqa: E731
        for name, mesh in ms.items():
            r = MeshRenderer(intr, dev)
            T_n = int(mesh.triangles.shape[0])
            eager = lambda: r.render(mesh, R, T, want=WANT)  # noqa: E731
            eager()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                r.render(mesh, R, T, want=WANT)
            nbytes = 64 * T_n + 16 * HW + 20 * HW
            src, dst = torch.empty(nbytes // 8, dtype=torch.float32, device=dev), torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
            variants = {"eager": eager, "graph": graph.replay, "copy": lambda: dst.copy_(src),
                        "eager_no_small": lambda: r.render(mesh, R, T, want=WANT, fuse_small=False)}
            if gauss is not None:
                variants["gaussians"] = gauss
            t = timed(variants, a.calls, a.warmup)
            t.update(triangles=T_n, copy_bytes=nbytes, hit_share=float((r.render(mesh, R, T)["depth"] > 0).float().mean()), status=r.status())
            res[name] = t
            del graph
        wall = []
        for _ in range(a.warmup + 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = eval_depth_l1(ms["room_0.1"], ms["room_0.1"], (poses + poses)[:8], intr)
            wall.append(1e3 * (time.perf_counter() - t0))
        res["eval_depth_l1_8_views_wall"] = stats(wall[a.warmup:])
        res["eval_depth_l1"] = {k_: v for k_, v in d.items() if k_ != "per_view"}
        out[size] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
