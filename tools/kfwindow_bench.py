#!/usr/bin/env python3
"""One keyframe decision per tracked frame -- median depth, overlap counts against the K window keyframes, keyframe test and
evictions, read back by the host -- through `monogs_amd.keyframe_window.KeyframeWindow` (1 memset + 8 launches + one 32-byte
read-back) against the composition the tracker runs (utils/slam_tracker.py:192-284,412-452: boolean indexing, `torch.median`,
`count_nonzero`, 4x4 inverses and `.item()` in Python loops) on the same GPU tensors.

One process, the two sides alternating; wall time per decision (both sides end in a host read-back, so wall time is what a
tracker waits for), median / min / max over --alternations windows of --calls decisions.  Prints one JSON line per case.

    python tools/kfwindow_bench.py [--cases 640x480:39000,1200x680:103000] [--K 8,10] [--calls 50] [--alternations 5]
"""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_decision(depth, opacity, cur, rows, poses, K, window_size, window_full, check_overlap, kf_cutoff=0.4, n_dont_touch=2):
    """The tracker's own sequence of torch calls (every comparison of a device scalar in an `if` is a host synchronisation)."""
    valid = torch.logical_and(depth > 0, opacity)
    median = depth[valid].median()

    def w2c(R, T):
        M = torch.eye(4, device=R.device)
        M[:3, :3], M[:3, 3] = R, T
        return M
    Ts = [w2c(R, T) for R, T in poses]
    create = True
    if check_overlap:
        union = torch.logical_or(cur, rows[0]).count_nonzero()
        inter = torch.logical_and(cur, rows[0]).count_nonzero()
        ratio = inter / union
        if K < window_size:
            create = bool(ratio < 0.9)
        else:
            dist = torch.norm((Ts[0] @ torch.linalg.inv(Ts[1]))[0:3, 3])
            create = bool((ratio < 0.9 and dist > 0.05 * median) or dist > 0.08 * median)
    lst = list(range(K + 1))
    to_remove = []
    for i in range(n_dont_touch, len(lst)):
        inter = torch.logical_and(cur, rows[i - 1]).count_nonzero()
        denom = min(cur.count_nonzero(), rows[i - 1].count_nonzero())
        if inter / denom <= (kf_cutoff if window_full else 0.4):
            to_remove.append(i)
    removed = []
    if to_remove:
        lst.remove(to_remove[-1])
        removed.append(to_remove[-1])
    if len(lst) > window_size:
        inv0 = torch.linalg.inv(Ts[0])
        scores = []
        for i in lst[n_dont_touch:]:
            inv_dists = []
            for j in lst[n_dont_touch:]:
                if i != j:
                    inv_dists.append(1.0 / (torch.norm((Ts[i] @ torch.linalg.inv(Ts[j]))[0:3, 3]) + 1e-6).item())
            scores.append(torch.sqrt(torch.norm((Ts[i] @ inv0)[0:3, 3])).item() * sum(inv_dists))
        removed.append(lst[n_dont_touch + max(range(len(scores)), key=scores.__getitem__)])
    return create, removed, float(median)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="640x480:39000,1200x680:103000", help="WxH:gaussians, comma separated")
    ap.add_argument("--K", default="8,10", help="window keyframes (the window size is the same number: a full window)")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--alternations", type=int, default=5)
    a = ap.parse_args()
    from monogs_amd.keyframe_window import KeyframeWindow, pack_visibility
    dev = "cuda:0"
    g = torch.Generator().manual_seed(1)
    for case in a.cases.split(","):
        size, P = case.split(":")
        W, H = (int(x) for x in size.split("x"))
        P = int(P)
        for K in (int(k) for k in a.K.split(",")):
            depth = (torch.rand(1, H, W, generator=g) * 4 + 0.5).to(dev)
            depth[:, :, :7] = 0.0
            opacity = torch.ones(1, H, W, device=dev)
            cur = torch.rand(P, generator=g) < 0.5
            rows = [(cur & (torch.rand(P, generator=g) < 0.8)) | (torch.rand(P, generator=g) < 0.1) for _ in range(K)]
            poses = [(torch.eye(3), torch.tensor([0.03 * i, 0.01 * i * i, 0.02 * i])) for i in range(K + 1)]
            vps = [types.SimpleNamespace(R=R.to(dev), T=T.to(dev)) for R, T in poses]
            w = KeyframeWindow(K, check_viewpoints_overlap=True)
            w.cur_kf_list = list(range(K, 0, -1))
            w.viewpoints = dict(zip(w.cur_kf_list, vps[1:]))
            for k, r in zip(w.cur_kf_list, rows):
                w.set_visibility(k, pack_visibility(r).to(dev))
            n_touched = cur.to(torch.int32).to(dev)
            cur_d, rows_d = cur.to(dev), [r.to(dev) for r in rows]
            poses_d = [(v.R, v.T) for v in vps]

            def ours():
                out, _ = w.launch(K + 1, vps[0], depth, opacity, n_touched)
                return w.decode(out.tolist())

            def theirs():
                return torch_decision(depth, opacity, cur_d, rows_d, poses_d, K, K, False, True)
            rec, ref = ours(), theirs()
            removed = [p for p in (rec.removed_by_cutoff, rec.removed_by_size) if p >= 0]
            agrees = (rec.create_kf, removed, rec.median_depth) == ref
            times = {"ours": [], "torch": []}
            for _ in range(a.alternations):
                for name, fn in (("ours", ours), ("torch", theirs)):
                    fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append(1e6 * (time.perf_counter() - t0) / a.calls)
            stat = lambda v: dict(median_us=round(sorted(v)[len(v) // 2], 1), min_us=round(min(v), 1), max_us=round(max(v), 1))  # noqa: E731
            o, t = stat(times["ours"]), stat(times["torch"])
            print(json.dumps(dict(width=W, height=H, gaussians=P, K=K, launches="1 memset + 8 kernels", read_back_bytes=32,
                                  ours=o, torch=t, same_decision=agrees, speedup=round(t["median_us"] / o["median_us"], 1),
                                  decision=dict(create_kf=rec.create_kf, removed=removed))), flush=True)
