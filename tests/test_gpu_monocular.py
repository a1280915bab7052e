"""Monocular operation on the MI355X: the RGB-only mode of the fused losses and the depth hypothesis of a keyframe without measured
depth against their float64 mirror (tests/monocular_mirror.py, tied to the reference's helpers by tests/test_monocular_host.py),
the bitwise tie of the RGB-only losses to the pinned RGB-D modes, capture, the back-projection override, the dataset switch and a
short monocular SLAM run against no-information baselines (pytest -m gpu)."""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import monocular_mirror as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLOSE = dict(rtol=1e-4, atol=1e-9)          # the bars of tests/test_gpu_losses.py for the RGB-D modes


def _grads(loss, xs):
    return torch.autograd.grad(loss, xs, allow_unused=True)


def _with_depth(vp, depth):
    d = dict(vars(vp))
    d["depth"] = depth
    return types.SimpleNamespace(**d)


# ---- 1. the RGB-only losses against the mirror ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", mm.SIZES)
@pytest.mark.parametrize("kind,init", [("tracking", False), ("mapping", False), ("mapping", True)])
def test_rgb_only_losses_against_the_mirror(native_lib, H, W, kind, init):
    from monogs_amd import fused_losses as F
    vp, render, rdepth, op = mm.loss_inputs(H, W, 0, DEV)
    assert not bool(vp.mask[3:6].any()) and vp.exposure_a.item() != 0.0
    if kind == "tracking":
        loss = F.get_loss_tracking_rgb(render, rdepth, op, vp)
    else:
        loss = F.get_loss_mapping_rgb(render, rdepth, vp, init=init)
    g_render, g_depth, g_a, g_b = _grads(loss, [render, rdepth, vp.exposure_a, vp.exposure_b])
    cpu = types.SimpleNamespace(**{k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in vars(vp).items()})
    ref, r_render, r_a, r_b = mm.loss_and_grads(kind, render.detach().cpu(), op.cpu(), cpu, init=init)
    print(f"{kind} init={init} {H}x{W}: loss {loss.item():.9g} mirror {ref.item():.9g}")
    assert float(ref) > 0 and torch.allclose(loss.detach().cpu().double(), ref, **CLOSE)
    assert torch.allclose(g_render.cpu().double(), r_render, **CLOSE), (g_render.cpu().double() - r_render).abs().max()
    assert g_depth is not None and g_depth.shape == rdepth.shape and not bool(g_depth.any())          # zero-filled, not garbage
    if init:
        assert g_a is None and g_b is None
    else:
        assert torch.allclose(g_a.cpu().double(), r_a, **CLOSE) and torch.allclose(g_b.cpu().double(), r_b, **CLOSE)


@pytest.mark.parametrize("H,W", mm.SIZES)
@pytest.mark.parametrize("tracking,init", [(True, False), (False, False), (False, True)])
def test_rgb_only_loss_grads_equal_the_autograd_loss(native_lib, tracking, init, H, W):
    """As tests/test_gpu_losses.py requires of the RGB-D pair: the two-launch path gives the autograd path's numbers."""
    from monogs_amd import fused_losses as F
    vp, render, rdepth, op = mm.loss_inputs(H, W, 31, DEV)
    loss = F.get_loss_tracking_rgb(render, rdepth, op, vp) if tracking else F.get_loss_mapping_rgb(render, rdepth, vp, init=init)
    ref = _grads(loss, [render] + ([] if init else [vp.exposure_a, vp.exposure_b]))
    lg = F.loss_grads(render, None, op if tracking else None, vp, tracking=tracking, init=init, rgb_only=True)
    assert torch.allclose(lg.loss, loss.detach(), rtol=1e-6, atol=0)
    assert torch.equal(lg.d_render, ref[0]) and lg.d_depth is None
    if init:
        assert lg.d_exposure_a is None
    else:
        assert torch.allclose(lg.d_exposure_a, ref[1], rtol=1e-5, atol=1e-9)
        assert torch.allclose(lg.d_exposure_b, ref[2], rtol=1e-5, atol=1e-9)
    # LossGrads.backward drives the colour image alone
    x = torch.rand(3, H, W, device=DEV, requires_grad=True)
    y = torch.rand(1, H, W, device=DEV, requires_grad=True)
    lg.backward(x * 2.0, y * 2.0, None)
    assert torch.equal(x.grad, lg.d_render * 2.0) and y.grad is None


# ---- 2. bitwise tie to the pinned modes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", mm.SIZES)
def test_rgb_only_tracking_is_the_tracking_mode_on_zero_depth(native_lib, H, W):
    from monogs_amd import fused_losses as F
    vp, render, rdepth, op = mm.loss_inputs(H, W, 2, DEV)
    a = F.get_loss_tracking_rgb(render, rdepth, op, vp)
    b = F.get_loss_tracking(render, rdepth, op, _with_depth(vp, torch.zeros(H, W, device=DEV)))
    assert torch.equal(a.detach(), b.detach()) and a.item() > 0
    assert torch.equal(_grads(a, [render])[0], _grads(b, [render])[0])


@pytest.mark.parametrize("H,W", mm.SIZES)
@pytest.mark.parametrize("init", [False, True])
def test_rgb_only_mapping_is_the_mapping_mode_at_lambda_one(native_lib, H, W, init):
    from monogs_amd import fused_losses as F
    vp, render, rdepth, _ = mm.loss_inputs(H, W, 3, DEV)
    a = F.get_loss_mapping_rgb(render, rdepth, vp, init=init)
    b = F.get_loss_mapping(render, rdepth, _with_depth(vp, torch.ones(H, W, device=DEV)), init=init, lambda_depth=1.0)
    assert torch.equal(a.detach(), b.detach()) and a.item() > 0
    assert torch.equal(_grads(a, [render])[0], _grads(b, [render])[0])
    # the gap being closed: without depth the RGB-D mapping loss is 0 / 0, the RGB-only one is a number
    nan = F.get_loss_mapping(render, rdepth, _with_depth(vp, torch.zeros(H, W, device=DEV)), init=init)
    assert math.isnan(nan.item()) and math.isfinite(a.item())


# ---- 3. the depth hypothesis against the mirror ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", mm.SIZES)
@pytest.mark.parametrize("seed", mm.SEEDS)
def test_pseudo_depth_against_the_mirror(native_lib, H, W, seed):
    from monogs_amd.monocular import pseudo_depth
    depth, opacity, valid_rgb, noise = mm.recipe(H, W, seed)
    m = mm.pseudo_depth(depth, opacity, valid_rgb, noise)
    args = (depth.to(DEV), opacity.to(DEV), valid_rgb.to(DEV))
    out, stats = pseudo_depth(*args, noise=noise.to(DEV))
    out2, stats2 = pseudo_depth(*args, noise=noise.to(DEV))
    assert torch.equal(out, out2) and torch.equal(stats, stats2)                     # bitwise reproducible
    out, (median, std, count, init) = out.cpu(), stats.cpu()
    rel = abs(float(std) - float(m["std"])) / float(m["std"])
    print(f"{H}x{W} seed {seed}: count {int(count)} median {float(median):.7f} std {float(std):.7f} (float64 {float(m['std']):.9f}, "
          f"rel {rel:.2e})  max |out - mirror| {(out.double() - m['depth']).abs().max().item():.2e}")
    assert int(count) == m["count"] and float(init) == 0.0
    assert torch.equal(median, depth[m["valid"]].median())                           # bit-equal to torch.median of the float32 selection
    assert rel <= 1e-5            # half the decision margin of these inputs (test_monocular_host.py): no decision can flip
    # the outlier set the kernel's own statistics decide in float32, against the mirror's
    outlier = (depth > median + std) | (depth < median - std) | ~m["valid"]
    assert torch.equal(outlier, m["outlier"])
    assert torch.allclose(out.double(), m["depth"], rtol=1e-5, atol=1e-6)
    assert bool((out[~valid_rgb] == 0).all()) and bool((out[valid_rgb] != 0).all())


# ---- 4. init rule and fallback -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", mm.SIZES)
def test_pseudo_depth_init_rule_and_fallback(native_lib, H, W):
    from monogs_amd.monocular import pseudo_depth
    depth, opacity, valid_rgb, noise = mm.recipe(H, W, 0)
    want = torch.where(valid_rgb, 2.0 + 0.3 * noise.double(), torch.zeros(H, W, dtype=torch.float64))
    z, ok = noise.to(DEV), valid_rgb.to(DEV)
    one = torch.zeros(H, W)
    one[H // 2, W // 2] = 2.5
    cases = dict(no_render=(None, None, 0), zero_opacity=(depth.to(DEV), torch.zeros(H, W, device=DEV), 0),
                 one_pixel=(one.to(DEV), torch.ones(H, W, device=DEV), 1 if bool(valid_rgb[H // 2, W // 2]) else 0))
    for name, (rd, ro, n) in cases.items():
        out, stats = pseudo_depth(rd, ro, ok, noise=z)
        assert torch.isfinite(out).all() and torch.isfinite(stats).all(), name
        assert stats.tolist() == [2.0, pytest.approx(0.3, rel=1e-7), float(n), 1.0], (name, stats.tolist())
        assert torch.allclose(out.cpu().double(), want, rtol=1e-6, atol=1e-7), name
        assert bool((out.cpu()[~valid_rgb] == 0).all()), name
    # no mask at all, drawn from a device generator: the same call twice gives the same image
    g = lambda: torch.Generator(device=DEV).manual_seed(5)  # noqa: E731
    a, _ = pseudo_depth(None, None, None, generator=g(), shape=(H, W))
    b, _ = pseudo_depth(None, None, None, generator=g(), shape=(H, W))
    assert a.shape == (H, W) and torch.equal(a, b) and 1.0 < float(a.mean()) < 3.0


# ---- 5. capture ----------------------------------------------------------------------------------------------------------------------
def test_pseudo_depth_and_rgb_only_loss_grads_replay_from_a_graph(native_lib):
    from monogs_amd import fused_losses as F
    from monogs_amd.monocular import pseudo_depth
    H, W = mm.SIZES[0]

    def inputs(seed):
        depth, opacity, valid_rgb, noise = (t.to(DEV) for t in mm.recipe(H, W, seed))
        vp, render, _, op = mm.loss_inputs(H, W, seed, DEV)
        return [depth, opacity, valid_rgb, noise, render.detach(), op, vp.rgb, vp.mask, vp.grad_mask]

    static = [t.clone() for t in inputs(0)]
    vp0 = mm.loss_inputs(H, W, 0, DEV)[0]

    def step(t):
        vp = types.SimpleNamespace(rgb=t[6], depth=vp0.depth, mask=t[7], grad_mask=t[8], exposure_a=vp0.exposure_a,
                                   exposure_b=vp0.exposure_b, sensor="monocular")
        pd, stats = pseudo_depth(t[0], t[1], t[2], noise=t[3])
        lg = F.loss_grads(t[4], None, t[5], vp, tracking=True, rgb_only=True)
        return pd, stats, lg.d_render, lg.scratch

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(static)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = step(static)
    for seed in (1, 2):
        fresh = inputs(seed)
        for dst, src in zip(static, fresh):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        want = step(fresh)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
        assert torch.equal(got[3][10:13], want[3][10:13])                # d(exposure a, b) and the loss value
        assert float(want[1][2]) > 2 and float(want[3][12]) > 0


# ---- 6. the back-projection override ---------------------------------------------------------------------------------------------
K_SMALL = dict(fx=535.4 / 4, fy=539.2 / 4, cx=320.1 / 4, cy=247.6 / 4, W=160, H=120)


def test_extend_from_frame_back_projects_the_given_depth(native_lib):
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.monocular import monocular_frames, pseudo_depth, valid_rgb
    from monogs_amd.sequences import make_room_sequence
    src, intr = make_room_sequence(2, K_SMALL, device=DEV)
    vp = monocular_frames(src)[1]
    assert vp.sensor == "monocular" and not bool(vp.depth.any())
    vp.update_RT(vp.R_gt, vp.T_gt)
    pd, _ = pseudo_depth(None, None, valid_rgb(vp.rgb), generator=torch.Generator(device=DEV).manual_seed(1))
    gmap = GaussianMap(DEV)
    assert gmap.extend_from_frame(vp, intr, downsample=8, init=True, point_size=1.0) == 0 and len(gmap) == 0      # depth >= 1e-3 nowhere
    n = gmap.extend_from_frame(vp, intr, downsample=8, init=True, point_size=1.0, depth=pd)
    assert n == len(gmap) == int(int((pd >= 1e-3).sum()) / 8) > 1000
    assert not bool(vp.depth.any())                                       # the viewpoint's own depth is untouched
    pc = gmap.get_xyz.detach().double() @ vp.R.double().t() + vp.T.double()
    u = intr.fx * pc[:, 0] / pc[:, 2] + intr.cx - 0.5
    v = intr.fy * pc[:, 1] / pc[:, 2] + intr.cy - 0.5
    ui, vi = u.round().long(), v.round().long()
    assert float((u - ui).abs().max()) < 1e-2 and float((v - vi).abs().max()) < 1e-2          # pixel centres
    assert bool(((ui >= 0) & (ui < 160) & (vi >= 0) & (vi < 120)).all())
    assert torch.allclose(pc[:, 2], pd[vi, ui].double(), rtol=1e-5, atol=0)
    assert torch.isfinite(gmap.get_scaling).all()


# ---- 7. the dataset switch ---------------------------------------------------------------------------------------------------------
def _quaternion(R):
    w = math.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2]) / 2.0
    return (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w


def test_dataset_frames_monocular(native_lib, tmp_path):
    from PIL import Image
    from monogs_amd.dataset import dataset_frames, load_dataset
    from monogs_amd.monocular import valid_rgb
    from monogs_amd.sequences import make_room_sequence
    k = dict(fx=535.4 / 8, fy=539.2 / 8, cx=320.1 / 8, cy=247.6 / 8, W=80, H=60)
    src, _ = make_room_sequence(12, k, device=DEV)
    os.makedirs(tmp_path / "rgb"), os.makedirs(tmp_path / "depth")
    lists = {n: ["# header", "# header", "# header"] for n in ("rgb", "depth", "groundtruth")}
    for i, f in enumerate(src):
        t = 100.0 + 0.04 * i
        rgb8 = (f.rgb.permute(1, 2, 0).cpu().double().numpy() * 255.0).round().clip(0, 255).astype(np.uint8)
        rgb8[:4] = 0                                                    # a black border, as an undistorted image brings one
        d16 = (f.depth.cpu().double().numpy() * 5000.0).round().clip(0, 65535).astype(np.uint16)
        Image.fromarray(rgb8).save(tmp_path / "rgb" / f"{t:.6f}.png")
        Image.fromarray(d16).save(tmp_path / "depth" / f"{t:.6f}.png")
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = f.R_gt.cpu().double().numpy(), f.T_gt.cpu().double().numpy()
        c2w = np.linalg.inv(w2c)
        lists["rgb"].append(f"{t:.6f} rgb/{t:.6f}.png")
        lists["depth"].append(f"{t:.6f} depth/{t:.6f}.png")
        lists["groundtruth"].append(" ".join(f"{v:.9f}" for v in (t, *c2w[:3, 3], *_quaternion(c2w[:3, :3]))))
    for n, rows in lists.items():
        (tmp_path / f"{n}.txt").write_text("\n".join(rows) + "\n")
    cal = dict(fx=k["fx"], fy=k["fy"], cx=k["cx"], cy=k["cy"], k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, distorted=False, width=80,
               height=60, depth_scale=5000.0, use_depth=True)
    config = dict(Dataset=dict(type="tum", dataset_path=str(tmp_path), Calibration=cal))
    depthless = dict(Dataset=dict(type="tum", dataset_path=str(tmp_path), Calibration=dict(cal, use_depth=False)))
    with pytest.raises(ValueError, match="RGB-D"):                      # the default still refuses a dataset without depth
        dataset_frames(load_dataset(depthless, device=DEV), 12, device=DEV)
    mono_cfg = dict(depthless, Training=dict(rgb_boundary_threshold=0.01))
    mono_cfg["Dataset"] = dict(depthless["Dataset"], sensor_type="monocular")
    runs = [dataset_frames(load_dataset(config, device=DEV), 12, device=DEV, monocular=True),      # depth files present: ignored
            dataset_frames(load_dataset(depthless, device=DEV), 12, device=DEV, monocular=True),
            dataset_frames(load_dataset(mono_cfg, device=DEV), 12, device=DEV, config=mono_cfg)]     # the YAML's sensor_type
    for frames, intr in runs:
        assert len(frames) == 12 and (intr.width, intr.height) == (80, 60)
        for f, s in zip(frames, src):
            assert f.sensor == "monocular" and f.depth.shape == (60, 80) and not bool(f.depth.any())
            assert f.mask.dtype == torch.bool and not bool((f.mask & ~valid_rgb(f.rgb)).any()) and not bool(f.mask[:4].any())
            assert bool(f.mask[4:].any())
            assert (f.R_gt - s.R_gt).abs().max() <= 1e-6 and (f.T_gt - s.T_gt).abs().max() <= 1e-6
        assert frames[0].depth.data_ptr() == frames[-1].depth.data_ptr()          # one shared zero image
    rgbd, _ = dataset_frames(load_dataset(config, device=DEV), 12, device=DEV)
    assert rgbd[0].sensor == "depth" and bool(rgbd[0].depth.any())


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------------
RUN = dict(kf_interval=2, tracking_itr_num=100, init_itr_num=150, mapping_itr_num=50, window_size=8)


@pytest.fixture(scope="module")
def room(native_lib):
    from monogs_amd.sequences import ROOM_SURFACES, make_room_sequence
    frames, intr = make_room_sequence(9, step_scale=4, device=DEV, with_segmentation=True)
    return frames, intr, ROOM_SURFACES


def _l1(vp, R, T, out):
    """L1 between the frame and a render of the final map from the pose (R, T)."""
    from monogs_amd.frames import Viewpoint
    from monogs_amd.mapping import render_map
    probe = Viewpoint(-1, vp.rgb, vp.depth, DEV, mask=vp.mask, grad_mask=vp.grad_mask, sensor="monocular")
    probe.update_RT(R.to(DEV), T.to(DEV))
    with torch.no_grad():
        return float((render_map(probe, out["intr"], out["map"], torch.zeros(3, device=DEV))["render"] - vp.rgb).abs().mean())


@pytest.mark.parametrize("graph", [False, True])
def test_monocular_run_beats_the_no_information_baselines(room, graph):
    """Conditions against no-information baselines, not measured bars (the figures measured on the MI355X are in DESIGN.md)."""
    from monogs_amd.monocular import monocular_frames
    from monogs_amd.slam_harness import run_slam
    frames, intr, n_obj = room
    mono = monocular_frames(frames)
    # (nr_objects: the run then hands its map and frames back, which the render condition needs)
    out = run_slam(sensor="monocular", sequence=(mono, intr), graph_tracking=graph, graph_mapping=graph, nr_objects=n_obj, **RUN)
    assert out["sensor"] == "monocular" and out["frames"] == 9 and out["keyframes"] == 5
    assert [s["frame"] for s in out["pseudo_depth_stats"]] == [0, 2, 4, 6, 8]
    assert [s["used_init_rule"] for s in out["pseudo_depth_stats"]] == [True, False, False, False, False]
    assert all(torch.isfinite(R).all() and torch.isfinite(T).all() for R, T in out["poses"])
    assert all(torch.isfinite(p).all() for p in out["map"].params()) and out["gaussians"] > 0
    assert not any(bool(f.depth.any()) for f in mono)
    for first, last in out["map_loss"]:
        assert math.isfinite(first) and last < first, out["map_loss"]
    l1 = [(i, _l1(mono[i], *out["poses"][i], out), _l1(mono[i], *out["poses"][i - 1], out)) for i in range(1, 9)]
    gt = torch.stack(out["camera_centers_gt"]).double()
    still = float(((gt - gt.mean(0)) ** 2).sum(1).mean().sqrt())          # what a tracker that never moved scores once aligned
    rot = [math.degrees(math.acos(max(-1.0, min(1.0, (float((f.R.cpu().double() @ f.R_gt.cpu().double().t()).trace()) - 1) / 2))))
           for f in mono]
    print(f"graph={graph}: ATE raw {out['ate_rmse_m']:.4f} m, Sim(3)-aligned {out['ate_sim3']['rmse']:.4f} m (never-moved baseline "
          f"{still:.4f} m), rotation error mean {sum(rot) / len(rot):.3f} max {max(rot):.3f} deg, {out['gaussians']} Gaussians, "
          f"map_loss {[(round(a, 4), round(b, 4)) for a, b in out['map_loss']]}, L1 own/previous pose "
          f"{[(i, round(a, 4), round(b, 4)) for i, a, b in l1]}, pseudo-depth {out['pseudo_depth_stats']}")
    for i, own, prev in l1:
        assert own < prev, (i, own, prev)
    assert out["ate_sim3"]["aligned"] and out["ate_sim3"]["correct_scale"] and out["ate_sim3"]["n"] == 9
    assert out["ate_sim3"]["rmse"] < still, (out["ate_sim3"]["rmse"], still)


def test_depth_run_keeps_its_result_keys(room):
    from monogs_amd.slam_harness import run_slam
    frames, intr, _ = room
    with open(os.path.join(GOLDEN, "run_slam_contract.json")) as f:
        recorded = {k for k in json.load(f)["eager"]["keys"] if "." not in k}
    out = run_slam(sensor="depth", sequence=(frames, intr), kf_interval=2, tracking_itr_num=4, init_itr_num=20, mapping_itr_num=4,
                   window_size=8)
    assert set(out) == recorded, sorted(set(out) ^ recorded)
    assert set(run_slam(sequence=(frames, intr), kf_interval=4, tracking_itr_num=2, init_itr_num=10, mapping_itr_num=2)) == recorded
    with pytest.raises(ValueError, match="monocular"):
        from monogs_amd.monocular import monocular_frames
        run_slam(sensor="depth", sequence=(monocular_frames(frames), intr), **RUN)


def test_a_window_that_mixes_sensors_is_refused(room):
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.mapping import WindowMapper
    from monogs_amd.monocular import monocular_frames
    frames, intr, _ = room
    for f in frames[:2]:
        f.update_RT(f.R_gt, f.T_gt)
    gmap = GaussianMap(DEV)
    gmap.extend_from_frame(frames[0], intr, downsample=32, init=True, point_size=1.0)
    mapper = WindowMapper(gmap, intr, torch.zeros(3, device=DEV))
    mapper.map_surgery = False
    with pytest.raises(ValueError, match="mixes"):
        mapper.optimize_map([frames[0], monocular_frames(frames[1:2])[0]], iters=1)
