#!/usr/bin/env python3
"""Device time of the TSDF fusion and of the mesh extraction (monogs_amd.tsdf, csrc/tsdf.hip) on the synthetic room:

  integrate   one frame (ground-truth depth + colour) at 640 x 480 and at 1200 x 680 into the 2 cm volume over the room
              (301 x 151 x 301 voxels, five planes), beside
  copy        a device copy that moves the bytes integrate must move -- five planes read and written for every voxel the frame
              updates, the four image planes read once -- and
  forward     the plain no-grad render of the same frame from a room map (what ``fuse_map`` pays per keyframe before it integrates);
  extract     count phase + the read-back of {V, T} + emit phase on the volume after six frames of the room sequence, with V and T;
              ``extract_count`` is the count phase alone (no read-back inside the bracket).

Every call is timed on its own with a pair of device events, after --warmup calls of each variant; the variants alternate call by
call and the figure is the median of --calls calls (min and max beside it).  Prints one JSON line.

    python tools/mesh_bench.py [--calls 30] [--warmup 3] [--voxel 0.02]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"640x480": "fr3_office", "1200x680": "replica"}
ROOM_LO, ROOM_HI = (-3.0, -1.5, -3.0), (3.0, 1.5, 3.0)


def stats(v):
    s = sorted(v)
    return {"median_us": round(1e3 * s[len(s) // 2], 1), "min_us": round(1e3 * s[0], 1), "max_us": round(1e3 * s[-1], 1)}


def timed(variants, calls, warmup):
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(calls):
        for k, fn in variants.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop))
    return {k: stats(v) for k, v in times.items()}


def room_map(vp, intr, dev):
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.mapping import WindowMapper
    bg = torch.zeros(3, device=dev)
    gmap = GaussianMap(dev)
    gmap.extend_from_frame(vp, intr, downsample=8, init=True, point_size=1.0)
    mapper = WindowMapper(gmap, intr, bg, window_size=8)
    mapper.map_surgery = False
    mapper.optimize_map([vp], iters=80, init=True)
    for p in gmap.params():
        p.grad = None
    return gmap, bg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--voxel", type=float, default=0.02)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_bench needs a GPU: there is no CPU path and no CPU number")
    from monogs_amd import _lib
    from monogs_amd.gaussian_optim import activate
    from monogs_amd.renderer import render
    from monogs_amd.sequences import make_room_sequence
    from monogs_amd.tsdf import TSDFVolume, mesh_stats
    dev = "cuda:0"
    lib = _lib.load()
    res = {"voxel": args.voxel, "calls": args.calls, "warmup": args.warmup}
    for size, intrinsics in SIZES.items():
        frames, intr = make_room_sequence(6, intrinsics, device=dev, step_scale=40)
        for f in frames:
            f.update_RT(f.R_gt.clone(), f.T_gt.clone())
        vp = frames[0]
        H, W = int(intr.height), int(intr.width)
        vol = TSDFVolume.for_bounds(ROOM_LO, ROOM_HI, args.voxel, dev)
        vol.integrate(vp.depth, vp, None, intr, rgb=vp.rgb)
        touched = int((vol.planes()[1] > 0).sum())
        nbytes = touched * 5 * 2 * 4 + 4 * H * W * 4
        src, dst = torch.empty(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)     # nbytes / 2 read, nbytes / 2 written
        gmap, bg = room_map(vp, intr, dev)
        with torch.no_grad():
            rot, scales3, opac = activate(gmap._rotation.detach(), gmap._scaling.detach(), gmap._opacity.detach())
            xyz, feat = gmap._xyz.detach(), gmap._rgb.detach()

            def forward():
                return render(vp, intr, xyz, rot, scales3, opac, feat, bg)

            variants = {"integrate": lambda: vol.integrate(vp.depth, vp, None, intr, rgb=vp.rgb), "copy": lambda: dst.copy_(src),
                        "forward": forward}
            r = timed(variants, args.calls, args.warmup)
        r.update(dims=list(vol.dims), voxels=vol.dims[0] * vol.dims[1] * vol.dims[2], updated_voxels=touched, algorithmic_bytes=nbytes,
                 gaussians=len(gmap))
        r["integrate_GBps"] = round(nbytes / (r["integrate"]["median_us"] * 1e-6) / 1e9, 1)
        r["copy_GBps"] = round(nbytes / (r["copy"]["median_us"] * 1e-6) / 1e9, 1)
        r["integrate_over_forward"] = round(r["integrate"]["median_us"] / r["forward"]["median_us"], 3)
        # extract: the volume after all six frames
        vol.reset()
        for f in frames:
            vol.integrate(f.depth, f, None, intr, rgb=f.rgb)
        nx, ny, nz = vol.dims
        scratch = torch.empty(lib.mgs_tsdf_extract_scratch_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def count():
            _lib.check(lib.mgs_tsdf_extract_count(C.byref(vol._vol), 1.0, scratch.data_ptr(), counts.data_ptr(), stream), "count")

        mesh = vol.extract()
        e = timed({"extract": vol.extract, "extract_count": count}, max(args.calls // 3, 5), 2)
        ms = mesh_stats(mesh)
        r.update(e, V=int(mesh.vertices.shape[0]), T=int(mesh.triangles.shape[0]), scratch_bytes=int(scratch.numel()),
                 boundary_edges=ms["boundary_edges"], non_manifold_edges=ms["non_manifold_edges"], area_m2=round(ms["area"], 2))
        res[size] = r
        del vol, scratch, src, dst, mesh
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
