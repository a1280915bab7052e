"""``eval_rendering`` and the ``refine_iters`` / ``eval_render`` wiring of ``run_slam`` on the GPU (pytest -m gpu).

Per-frame bars: PSNR within 4.4e-5 dB of a float64 evaluation of the same render (the MSE bar of tests/test_gpu_metrics.py,
1e-5 relative), SSIM within the value bar of tests/test_gpu_ssim.py (1e-4 absolute) of the float64 checker of
tests/ssim_oracle.py."""
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def scene(native_lib):
    """Twelve frames of the synthetic sequence and a map back-projected from the first (nothing here optimises it)."""
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.slam_harness import make_sequence
    frames, intr = make_sequence(12, "fr3_office", n_gaussians=20000, device=DEV)
    for f in frames:
        f.update_RT(f.R_gt.clone(), f.T_gt.clone())
    gmap = GaussianMap(DEV)
    gmap.extend_from_frame(frames[0], intr, downsample=8, init=True, point_size=1.0)
    return frames, intr, gmap, torch.zeros(3, device=DEV)


def _reference_rows(frames, intr, gmap, bg, idx):
    """(psnr, ssim) per frame in float64 from the same render, by plain torch."""
    from ssim_oracle import ssim_ref
    from monogs_amd.gaussian_optim import activate
    from monogs_amd.renderer import render
    rows = []
    with torch.no_grad():
        rot, scales3, opac = activate(gmap._rotation.detach(), gmap._scaling.detach(), gmap._opacity.detach())
        for i in idx:
            image = render(frames[i], intr, gmap._xyz.detach(), rot, scales3, opac, gmap._rgb.detach(), bg)["render"]
            c, gt = torch.clamp(image, 0.0, 1.0), frames[i].rgb
            mask = gt > 0
            mse = float(((c.double() - gt.double())[mask] ** 2).mean())
            rows.append((20.0 * math.log10(1.0 / math.sqrt(mse)), float(ssim_ref(c.cpu(), gt.cpu(), "valid")), int(mask.sum())))
    return rows


# (frames handed over, keyframes, interval) -> range(0, n - 1, interval) without the keyframes.  The first case evaluates
# NOTHING: with 11 frames the reference's range stops at frame 5, and 0 and 5 are keyframes.
@pytest.mark.parametrize("n,kf,interval,want", [(11, (0, 5), 5, []), (12, (0, 5), 5, [10]), (12, (5,), 5, [0, 10]),
                                                (12, (0, 3, 6), 3, [9])])
def test_eval_rendering_frames_and_values(scene, tmp_path, n, kf, interval, want):
    from monogs_amd.evaluation import eval_rendering
    frames, intr, gmap, bg = scene
    out = eval_rendering(frames[:n], gmap, intr, bg, kf, interval=interval, save_dir=str(tmp_path))
    assert out["frames"] == want and [r["frame"] for r in out["per_frame"]] == want
    assert "mean_lpips" not in out
    assert out["stats"]["readbacks"] == (1 if want else 0) and out["stats"]["renders"] == len(want)
    saved = json.load(open(tmp_path / "psnr" / "final" / "final_result.json"))
    if not want:
        assert math.isnan(out["mean_psnr"]) and math.isnan(out["mean_ssim"])
        return
    ref = _reference_rows(frames, intr, gmap, bg, want)
    for got, (psnr, ssim, count) in zip(out["per_frame"], ref):
        d_psnr, d_ssim = abs(got["psnr"] - psnr), abs(got["ssim"] - ssim)
        print(f"frame {got['frame']}: psnr {got['psnr']:.4f} dB (err {d_psnr:.3g}, bar 4.4e-5), ssim {got['ssim']:.6f} (err {d_ssim:.3g}, "
              f"bar 1e-4), {got['count']} of {3 * intr.height * intr.width} elements counted")
        assert got["count"] == count and count > 0
        assert d_psnr <= 4.4e-5 and d_ssim <= 1e-4
    assert abs(out["mean_psnr"] - sum(r[0] for r in ref) / len(ref)) <= 4.4e-5
    assert abs(out["mean_ssim"] - sum(r[1] for r in ref) / len(ref)) <= 1e-4
    assert saved == dict(mean_psnr=out["mean_psnr"], mean_ssim=out["mean_ssim"])


# tests/test_gpu_slam.py's configuration at the fewest frames that leave ``eval_rendering`` one to look at (frame 5: every
# second frame is a keyframe, and range(0, n - 1, 5) reaches 5 from n = 7 -- the length its two-process test runs)
CFG = dict(n_frames=7, intrinsics="fr3_office", tracking_itr_num=100, mapping_itr_num=30, window_size=8, kf_interval=2,
           init_itr_num=80, n_gaussians=30000)
OLD_KEYS = {"kf_extend_s", "track_capture_s", "track_s", "track_iters", "tracked", "map_s", "map_iters", "keyframes", "renders",
            "surgery", "frames", "gaussians", "width", "height", "tracking_fps", "tracking_iters_per_s", "mapping_iters_per_s",
            "mapping_kf_per_s", "tracking_steady_iters_per_s", "mapping_steady_iters_per_s", "mapping_keyframe_iters_per_s",
            "mapping_replays", "mapping_eager_iters", "mapping_captures", "mapping_capture_s", "window_sizes", "kf_extend_ms",
            "ate_rmse_m", "track_iters_per_frame", "poses", "position_error_m", "camera_centers", "camera_centers_gt", "map_loss",
            "graph_tracking", "graph_mapping", "map_surgery", "config"}
NEW_KEYS = {"eval", "ate", "refinement"}


def _finite(v):
    return isinstance(v, (int, float)) and math.isfinite(v)


def test_run_slam_reports_refinement_and_evaluation(native_lib):
    from monogs_amd import rasterizer
    from monogs_amd.slam_harness import run_slam
    r = run_slam(graph_tracking=True, graph_mapping=True, refine_iters=40, eval_render=True, **CFG)
    assert set(r) == OLD_KEYS | NEW_KEYS, set(r) ^ (OLD_KEYS | NEW_KEYS)
    assert set(r["eval"]) == {"before_opt", "final"}
    for tag in ("before_opt", "final"):
        e = r["eval"][tag]
        assert e["frames"] == [5] and e["stats"]["readbacks"] == 1
        assert _finite(e["mean_psnr"]) and _finite(e["mean_ssim"]) and 0.0 < e["mean_ssim"] <= 1.0 and e["mean_psnr"] > 0.0, e
    assert r["ate"]["n"] == 4 and all(_finite(r["ate"][k]) for k in ("rmse", "mean", "median", "min", "max")), r["ate"]
    assert r["ate"]["aligned"] is False and r["ate"]["min"] <= r["ate"]["median"] <= r["ate"]["max"] and r["ate"]["rmse"] >= r["ate"]["mean"]
    ref = r["refinement"]
    assert ref["iters"] == 40 and ref["window"] == 10 and _finite(ref["it_per_s"]) and ref["it_per_s"] > 0
    assert ref["stats"]["eager_iters"] == 1 and ref["stats"]["replays"] == 39 and ref["stats"]["captures"] >= 1, ref["stats"]
    assert all(_finite(v) for part in (ref["first"], ref["last"]) for v in part.values()), ref
    print(f"eval before / after 40 refinement iterations: psnr {r['eval']['before_opt']['mean_psnr']:.3f} -> "
          f"{r['eval']['final']['mean_psnr']:.3f} dB, ssim {r['eval']['before_opt']['mean_ssim']:.4f} -> "
          f"{r['eval']['final']['mean_ssim']:.4f}; ate {r['ate']['rmse']:.3g} m; {ref['it_per_s']:.0f} it/s")
    assert not rasterizer.check_overflow()
    for k in ("poses", "camera_centers", "camera_centers_gt"):
        r.pop(k)
    json.dumps(r)                                                           # what tools/slam_bench.py prints


def test_run_slam_defaults_return_the_old_keys(native_lib):
    from monogs_amd.slam_harness import run_slam
    r = run_slam(graph_tracking=True, graph_mapping=True, **CFG)
    assert set(r) == OLD_KEYS, set(r) ^ OLD_KEYS
