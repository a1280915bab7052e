#!/usr/bin/env python3
"""Device time of the reconstruction evaluation (monogs_amd.mesh_eval, csrc/mesheval.hip) with points on the room mesh:

  nearest     one ``nearest_distance`` call at Q = P = 2e4 (both paths, forced) and at Q = P = 2e5 (the Morton-box path; the all-pairs
              figure at that size is the small one extrapolated as Q x P), queries and targets two different draws of ``sample_mesh``;
  copy        a device copy of the bytes the call must read and write (both point sets in, d2 out);
  ckdtree     wall time of ``scipy.spatial.cKDTree(targets).query(queries, workers=16)`` on the same points (build + query);
  sample      one ``sample_mesh`` launch sequence of 2e5 points (no read-back inside the bracket);
  eval        a whole ``eval_reconstruction`` of the room mesh against itself, 2e5 samples each (host wall time, its one read-back
              included).

Every device figure is a pair of events around one call, after --warmup calls of each variant; variants alternate call by call
and the figure is the median of --calls calls (min and max beside it).  Prints one JSON line.

    python tools/mesh_eval_bench.py [--calls 20] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_eval_bench needs a GPU: there is no CPU path to time")
    from scipy.spatial import cKDTree
    from monogs_amd import mesh_eval as ME
    from monogs_amd.sequences import room_mesh
    dev = "cuda:0"
    mesh = room_mesh(dev)
    out = {"grid_min": ME.nn_grid_min(), "room_mesh": dict(vertices=int(mesh.vertices.shape[0]), triangles=int(mesh.triangles.shape[0]))}
    for n in (20_000, 200_000):
        q, t = ME.sample_mesh(mesh, n, seed=1), ME.sample_mesh(mesh, n, seed=2)
        d2 = torch.empty(n, dtype=torch.float32, device=dev)
        src, dst = torch.cat([q.reshape(-1), t.reshape(-1), d2]), torch.empty(7 * n, dtype=torch.float32, device=dev)
        variants = {"morton": lambda: ME.nearest_distance(q, t, path="morton"), "copy": lambda: dst.copy_(src)}
        if n == 20_000:
            variants["all_pairs"] = lambda: ME.nearest_distance(q, t, path="all_pairs")
        r = timed(variants, a.calls, a.warmup)
        r["copy_bytes"] = 2 * 7 * n * 4
        if n == 20_000:
            assert torch.equal(ME.nearest_distance(q, t, path="morton"), ME.nearest_distance(q, t, path="all_pairs"))
            out["all_pairs_us_per_pair"] = r["all_pairs"]["median_us"] / (n * n)
        else:
            r["all_pairs_extrapolated_us"] = round(out["all_pairs_us_per_pair"] * n * n, 1)
        qc, tc = q.cpu().numpy(), t.cpu().numpy()
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            dk, _ = cKDTree(tc).query(qc, workers=16)
            wall.append(1e3 * (time.perf_counter() - t0))
        r["ckdtree_16_workers"] = stats(wall)
        got = ME.nearest_distance(q, t).sqrt().cpu().numpy()
        r["max_abs_difference_to_ckdtree_m"] = float(abs(got - dk).max())
        out[f"nearest_{n}"] = r
    n = 200_000
    out["sample_200000"] = timed({"sample": lambda: ME._sample_launch(mesh, n, 3, None, False)}, a.calls, a.warmup)["sample"]
    wall = []
    for i in range(a.warmup + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ME.eval_reconstruction(mesh, mesh, n_samples=n)
        wall.append(1e3 * (time.perf_counter() - t0))
    out["eval_200000_wall"] = stats(wall[a.warmup:])
    out["eval_figures"] = {k: v for k, v in res.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
