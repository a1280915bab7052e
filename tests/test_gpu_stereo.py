"""``mgs_stereo_depth`` on the device against the integer mirror (tests/stereo_mirror.py): the rectified images, the aggregated
volume S (through ``sum_out``), ``disp16``, ``depth`` and ``rgb`` are compared BIT FOR BIT -- everything up to disp16 is integer,
and the depth step is one IEEE double division rounded to float32, which the device does as the host does.  The shapes are the
smallest at which each part can go wrong: valid widths and heights at or below the window, a single valid column, every D the
entry point takes (lanes beyond D idle in the path and winner kernels), odd sizes, one row."""
import csv
import functools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import stereo_mirror as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "euroc_calibration.json")))
DEV = "cuda:0"

#        W,   H,  D, block
SHAPES = [(96, 24, 64, 20),      # the valid width (32) and the height near the window size
          (65, 8, 64, 20),       # one valid column: every path has length 1, the window is fully clamped
          (80, 33, 16, 5),       # small D, small window
          (117, 37, 32, 20),     # odd sizes
          (130, 3, 48, 9),       # few rows, D = 48
          (70, 1, 64, 20)]       # H = 1
REFERENCE = dict(uniqueness_ratio=40)                               # with block 20 and D 64: the reference's matcher
LENIENT = dict(uniqueness_ratio=0, disp12_max_diff=64)              # nearly every pixel valid: sub-pixel, table and median see data
MIXED = dict(uniqueness_ratio=5)                                    # on noise: the uniqueness test and the left-right check each
                                                                    # reject a part of the pixels (the mirror: 18-70 % stay valid)


def _noise(W, H, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)


def _smooth(W, H, seed):
    """A textured pair with a true disparity of 3 and some noise: what the lenient settings make valid depth of."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, W + 8)).astype(np.float64)
    base = (base + np.roll(base, 1, axis=1) + np.roll(base, 1, axis=0)) / 3.0
    right = base[:, 3:W + 3] + rng.normal(0, 2, (H, W))
    left = base[:, :W] + rng.normal(0, 2, (H, W))
    return left.clip(0, 255).astype(np.uint8), right.clip(0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(left, right, D, matcher keywords, maps or None) of a named case; the arrays are shared and never written."""
    kind, _, idx = name.partition(":")
    if kind in ("noise", "lenient", "smooth", "mixed"):
        W, H, D, block = SHAPES[int(idx)]
        left, right = (_smooth if kind == "smooth" else _noise)(W, H, 10 + int(idx))
        return left, right, D, dict(dict(noise=REFERENCE, mixed=MIXED).get(kind, LENIENT), block_size=block), None
    if kind == "stereogram":
        left, right, _ = sm.stereogram()
        return left, right, 32, dict(REFERENCE, block_size=20), None
    if kind == "constant":
        return np.full((8, 40), 255, np.uint8), np.zeros((8, 40), np.uint8), 16, dict(uniqueness_ratio=0, block_size=20), None
    if kind == "rectify":
        from monogs_amd.stereo import calibration_maps
        W, H, D = 117, 37, 32
        s = W / 752.0
        cal = json.loads(json.dumps(FIXTURE["Calibration"]))
        for cam in ("cam0", "cam1"):
            for which in ("raw", "opt"):
                for k in ("fx", "fy", "cx", "cy"):
                    cal[cam][which][k] *= s
        cal["width"], cal["height"] = W, H
        maps = [m.copy() for m in calibration_maps(cal)]
        if idx == "outside":                                        # no map value may read outside the source
            maps[0][:, :9] -= 40.0
            maps[3][-6:, :] += 9.5
            maps[2][5, 40:48] = (np.nan, np.inf, -np.inf, 1e30, -1e30, -1.0, -0.5, float(W) - 0.5)
            maps[1][7, 50:54] = (np.nan, float(H) - 1.0, float(H), -1.02)
        left, right = _smooth(W, H, 77)
        return left, right, D, dict(LENIENT, block_size=20), tuple(maps)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _expected(name):
    left, right, D, kw, maps = _case(name)
    return sm.stereo(left, right, D=D, maps=maps, **kw)


def _run(name, debug=True, matcher=None, scratch=None):
    from monogs_amd.stereo import StereoMatcher
    left, right, D, kw, maps = _case(name)
    H, W = left.shape
    m = matcher or StereoMatcher(W, H, DEV, num_disparities=D, **kw)
    dbg = {} if debug else None
    dmaps = None if maps is None else tuple(torch.from_numpy(a).to(DEV) for a in maps)
    disp16, depth, rgb = m.compute(torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV), dmaps, debug=dbg, scratch=scratch)
    return disp16, depth, rgb, dbg


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(name, disp16, depth, rgb, dbg=None):
    exp = _expected(name)
    torch.cuda.synchronize()
    if dbg is not None:
        assert np.array_equal(dbg["rect_l"].cpu().numpy(), exp["rect_l"]), name
        assert np.array_equal(dbg["rect_r"].cpu().numpy(), exp["rect_r"]), name
        S = dbg["S"].cpu().numpy().astype(np.int64)
        bad = np.argwhere(S != exp["S"])
        assert bad.size == 0, (name, "S differs at", bad[:5].tolist(), len(bad), "of", S.size)
    got = disp16.cpu().numpy()
    bad = np.argwhere(got != exp["disp16"])
    assert bad.size == 0, (name, "disp16 differs at", bad[:5].tolist(), len(bad), [int(got[tuple(b)]) for b in bad[:5]],
                           [int(exp["disp16"][tuple(b)]) for b in bad[:5]])
    assert np.array_equal(_bits(depth.cpu().numpy()), _bits(exp["depth"])), name
    assert np.array_equal(_bits(rgb.cpu().numpy()), _bits(exp["rgb"])), name
    return exp


@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_noise_with_the_reference_matcher(idx):
    exp = _check(f"noise:{idx}", *_run(f"noise:{idx}"))
    D = SHAPES[idx][2]
    valid = exp["disp16"][:, D:] >= 0
    print(SHAPES[idx], "valid fraction", valid.mean())
    if SHAPES[idx][1] >= 3 and SHAPES[idx][0] - D >= 16:
        assert valid.mean() < 0.5                                   # the uniqueness test is what runs here


@pytest.mark.parametrize("kind", ["lenient", "smooth", "mixed"])
@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_valid_data_reaches_subpixel_table_and_median(kind, idx):
    exp = _check(f"{kind}:{idx}", *_run(f"{kind}:{idx}"))
    d = exp["disp16"][:, SHAPES[idx][2]:]
    print(kind, SHAPES[idx], "valid fraction", (d >= 0).mean(), "with a fraction", ((d >= 0) & (d % 16 != 0)).mean())
    if kind == "smooth" and SHAPES[idx][0] - SHAPES[idx][2] >= 16:
        assert (d >= 0).mean() > 0.5 and ((d >= 0) & (d % 16 != 0)).any()
    if kind == "mixed" and SHAPES[idx][0] - SHAPES[idx][2] >= 16:
        assert 0.1 < (d >= 0).mean() < 0.9


def test_stereogram():
    exp = _check("stereogram:", *_run("stereogram:"))
    _, _, gt = sm.stereogram()
    keep = sm.in_plane(gt, 32, 160)
    d = exp["disp16"][:, keep]
    assert (d >= 0).all() and np.abs(d / 16.0 - gt[keep][None, :]).max() <= 0.5


def test_constant_pair_needs_more_than_16_bits():
    disp16, depth, rgb, dbg = _run("constant:")
    _check("constant:", disp16, depth, rgb, dbg)
    assert (dbg["S"] == 562275).all() and (disp16[:, 16:] == 0).all()


@pytest.mark.parametrize("which", ["fixture", "outside"])
def test_rectified_pair(which):
    exp = _check(f"rectify:{which}", *_run(f"rectify:{which}"))
    left = _case(f"rectify:{which}")[0]
    assert not np.array_equal(exp["rect_l"], left)                  # (the maps did something)
    if which == "outside":
        assert (exp["rect_l"][:, :5] == 0).all() and (exp["rect_r"][5, 40:45] == 0).all()


def test_without_sum_out_the_disparities_are_the_same():
    _check("smooth:3", *_run("smooth:3", debug=False)[:3])
    _check("noise:0", *_run("noise:0", debug=False)[:3])


def test_two_streams_with_separate_scratch_agree():
    from monogs_amd.stereo import StereoMatcher
    names = ("smooth:0", "lenient:0")                               # the same size: 96 x 24 x 64
    W, H, D, _ = SHAPES[0]
    matchers = [StereoMatcher(W, H, DEV, num_disparities=D, **_case(n)[3]) for n in names]
    streams = [torch.cuda.Stream() for _ in names]
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):                                              # interleaved: each stream is busy while the other is fed
        for n, m, s in zip(names, matchers, streams):
            with torch.cuda.stream(s):
                outs.append((n, _run(n, matcher=m)))
    torch.cuda.synchronize()
    assert matchers[0].scratch.data_ptr() != matchers[1].scratch.data_ptr()
    for n, o in outs:
        _check(n, *o)


def test_captured_graph_replay_agrees():
    from monogs_amd.stereo import StereoMatcher
    name = "smooth:3"
    left, right, D, kw, _ = _case(name)
    H, W = left.shape
    m = StereoMatcher(W, H, DEV, num_disparities=D, **kw)
    dl, dr = torch.zeros(H, W, dtype=torch.uint8, device=DEV), torch.zeros(H, W, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.compute(dl, dr)                                           # warm-up: allocates the scratch outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                       # a linear chain of twelve kernel nodes
        out = m.compute(dl, dr)
    dl.copy_(torch.from_numpy(left))
    dr.copy_(torch.from_numpy(right))
    g.replay()
    _check(name, *out)


def test_argument_errors_launch_nothing():
    from monogs_amd.stereo import StereoMatcher
    name = "noise:2"
    left, right, D, kw, _ = _case(name)
    H, W = left.shape
    good = _run(name)
    torch.cuda.synchronize()
    for bad in (dict(block_size=64), dict(p2=1 << 21), dict(uniqueness_ratio=101), dict(pre_filter_cap=200), dict(bf=float("nan"))):
        m = StereoMatcher(W, H, DEV, num_disparities=D, **dict(kw, **bad))
        with pytest.raises(Exception, match="mgs_stereo_depth"):
            m.compute(torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV))
    m = StereoMatcher(W, H, DEV, num_disparities=D, **kw)
    with pytest.raises(ValueError, match="left_u8 must be"):
        m.compute(torch.from_numpy(left), torch.from_numpy(right).to(DEV))
    with pytest.raises(ValueError, match="four tensors"):
        m.compute(torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV), maps=(torch.zeros(H, W, device=DEV),) * 2)
    torch.cuda.synchronize()
    _check(name, *good)
    _check(name, *_run(name, matcher=m))


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _write_euroc(folder, pairs):
    t0 = 1403636579763555584
    for cam in (0, 1):
        os.makedirs(folder / "mav0" / f"cam{cam}" / "data")
        for i, pair in enumerate(pairs):
            Image.fromarray(pair[cam]).save(folder / "mav0" / f"cam{cam}" / "data" / f"{t0 + i * 50_000_000}.png")
    with open(folder / "mav0" / "cam0" / "sensor.yaml", "w") as f:
        f.write("sensor_type: camera\nT_BS:\n  cols: 4\n  rows: 4\n  data: [" + ", ".join(repr(v) for row in FIXTURE["T_BS"] for v in row) + "]\n")
    os.makedirs(folder / "mav0" / "state_groundtruth_estimate0")
    with open(folder / "mav0" / "state_groundtruth_estimate0" / "data.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["#timestamp", "p_x", "p_y", "p_z", "q_w", "q_x", "q_y", "q_z"])
        for k in range(len(pairs)):
            w.writerow([t0 + k * 50_000_000 + 1000, 0.1 * k, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0])


def test_euroc_folder_to_viewpoints(tmp_path):
    from monogs_amd.dataset import dataset_frames
    from monogs_amd.frame_ingest import grad_mask
    from monogs_amd.stereo import load_stereo_dataset
    H, W, D = 48, 160, 32
    left, right, gt = sm.stereogram(H, W, seed=0)
    left2, right2, _ = sm.stereogram(H, W, seed=5)
    _write_euroc(tmp_path, [(left, right), (left2, right2)])
    cal = dict(FIXTURE["Calibration"], width=W, height=H, distorted=False)
    cfg = dict(Dataset=dict(type="euroc", sensor_type="stereo", dataset_path=str(tmp_path), start_idx=0, Calibration=cal,
                            Stereo=dict(num_disparities=D)))
    ds = load_stereo_dataset(cfg, device=DEV)
    d0 = ds[0]
    assert set(d0) == {"rgb", "depth", "mask", "grad_mask", "segmentation", "pose", "disp16"} and d0["segmentation"] is None
    assert d0["mask"].dtype == torch.bool and bool(d0["mask"].all()) and tuple(d0["mask"].shape) == (H, W)
    assert d0["grad_mask"].dtype == torch.bool and torch.equal(d0["grad_mask"], grad_mask(d0["rgb"]))
    _check("stereogram:", d0["disp16"], d0["depth"], d0["rgb"])
    frames, intr = dataset_frames(ds, 2, device=DEV)
    assert len(frames) == 2 and (intr.width, intr.height) == (W, H) and intr.fx == cal["cam0"]["opt"]["fx"]
    keep = sm.in_plane(gt, D, W)
    for f in frames:
        assert tuple(f.rgb.shape) == (3, H, W) and f.rgb.dtype == torch.float32 and f.depth.dtype == torch.float32
        z = f.depth.cpu().numpy()[:, keep].astype(np.float64)
        assert (z > 0).all()
        # |disparity - gt| <= 0.5 (the bound of the host test), seen through depth = bf / disparity; 1e-5 covers the float32 store
        assert np.abs(FIXTURE["bf"] / z - gt[keep][None, :]).max() <= 0.5 + 1e-5
    pose = torch.from_numpy(ds.poses[1]).to(torch.float32).to(DEV)
    assert torch.equal(frames[1].R_gt, pose[:3, :3]) and torch.equal(frames[1].T_gt, pose[:3, 3])
