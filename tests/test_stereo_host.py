"""The stereo front end without a GPU: the specification's mirror (tests/stereo_mirror.py) on a stereogram with a known answer and
on the constant pair that overflows 16 bits, ``rectify_map`` against known answers, the EuRoC parser and dataset on a folder
written here, and the C ABI's refusals (nothing is launched)."""
import csv
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import stereo_mirror as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "euroc_calibration.json")))
PTR = 0x1000                          # non-NULL, 16-byte aligned and never dereferenced
FR1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628,
           k3=1.163314)


def _err(lib):
    return lib.mgs_last_error().decode()


# ---- the specification -------------------------------------------------------------------------------------------------------
def test_stereogram_every_in_plane_pixel_is_valid_and_within_half_a_disparity():
    """The true disparity has C = 0 (the left view is a shifted copy of the right one), so it is the integer minimum, and the
    parabola's vertex lies within half a disparity of it: |disp16 / 16 - gt| <= 0.5, no pixel excused."""
    H, W, D = 48, 160, 32
    left, right, gt = sm.stereogram(H, W, seed=0)
    out = sm.stereo(left, right, D=D, block_size=20)
    keep = sm.in_plane(gt, D, W)
    assert int(keep.sum()) * H == 3840
    d = out["disp16"][:, keep].astype(np.float64)
    err = np.abs(d / 16.0 - gt[keep][None, :])
    print("in-plane pixels", d.size, "invalid", int((d < 0).sum()), "max error", err.max())
    assert (d >= 0).all()
    assert err.max() <= 0.5
    cols = np.nonzero(keep)[0]
    inner = cols[cols + 12 <= W - 1]                        # (the pre-filter pins P to ftzero at x = W - 1 in the left view only)
    assert (out["C"][:, inner - D, gt[inner]] == 0).all()
    z = out["depth"][:, keep]
    assert z.dtype == np.float32 and (np.abs(sm.EUROC_BF / z - gt[keep][None, :]) <= 0.5 + 1e-4).all()


def test_constant_pair_does_not_fit_16_bits_and_ties_go_to_the_lowest_disparity():
    """255 against 0: every pixel cost is 255 (the pre-filtered images are flat), C = 21^2 x 255 = 112 455 and S = 5 C = 562 275
    everywhere -- any 16-bit volume wraps.  Every disparity ties: the lowest wins, each right-view column has one claimant."""
    H, W, D = 8, 40, 16
    left, right = np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8)
    out = sm.stereo(left, right, D=D, block_size=20, uniqueness_ratio=0)
    assert (out["pc"] == 255).all()
    assert (out["C"] == 112455).all() and 112455 > 65535
    assert (out["S"] == 562275).all()
    assert (out["disp16"][:, D:] == 0).all() and (out["disp16"][:, :D - 1] == -16).all()
    assert (out["depth"][:, D:] == np.float32(sm.EUROC_BF / 1e10)).all() and (out["depth"][:, :D - 1] == 0).all()
    d16, disp2 = sm.winner(out["S"], W, 0)
    assert (d16[:, D:] == 0).all() and (disp2[:, D:] == 0).all() and (disp2[:, :D] == -1).all()


def test_equal_costs_in_the_right_view_table_go_to_the_largest_x():
    """Two pixels of one row claim the same right-view column with the same cost: x = D + 9 with d = 5 and x = D + 7 with d = 3.
    The row is walked from the right, and only a strictly lower cost replaces an entry: the table keeps d = 5."""
    H, W, D = 2, 16 + 12, 16
    S = np.full((H, W - D, D), 1000, dtype=np.int64)
    S[0, 9, 5] = S[0, 7, 3] = 10
    S[1, 9, 5], S[1, 7, 3] = 10, 9                          # (and a strictly lower cost does replace it)
    _, disp2 = sm.winner(S, W, 0)
    assert disp2[0, D + 4] == 5 and disp2[1, D + 4] == 3
    # the lowest d among equal minima
    S = np.full((1, 4, D), 7, dtype=np.int64)
    S[0, :, 2] = S[0, :, 11] = 3
    d16, _ = sm.winner(S, 4 + D, 0)
    assert (d16[0, D:] >> 4 == 2).all()


def test_subpixel_division_truncates_toward_zero():
    D = 16
    S = np.full((1, 1, D), 100, dtype=np.int64)
    S[0, 0, 4:7] = (31, 20, 30)                             # den = 21, numerator 16 + 21 = 37 -> 37 / 42 = 0
    assert sm.winner(S, 1 + D, 0)[0][0, D] == 80
    S[0, 0, 4:7] = (30, 20, 50)                             # den = 40, numerator -320 + 40 = -280 -> -280 / 80 = -3 (not -4)
    assert sm.winner(S, 1 + D, 0)[0][0, D] == 77


def test_defaulting_follows_opencv():
    assert sm.defaults(block_size=20) == dict(s=10, P1=2, P2=5, uniq=40, max_diff=1, ftzero=15)
    assert sm.defaults(block_size=0, p1=8, p2=3, uniqueness_ratio=-1, disp12_max_diff=7, pre_filter_cap=30) == \
        dict(s=2, P1=8, P2=9, uniq=10, max_diff=7, ftzero=31)


# ---- rectify_map -------------------------------------------------------------------------------------------------------------
def _K(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def test_rectify_map_equals_undistort_map_without_rotation():
    from monogs_amd.frame_ingest import undistort_map
    from monogs_amd.stereo import rectify_map
    s = 1.0 / 8.0
    K = _K(FR1["fx"] * s, FR1["fy"] * s, FR1["cx"] * s, FR1["cy"] * s)
    dist = [FR1[k] for k in ("k1", "k2", "p1", "p2", "k3")]
    mx, my = rectify_map(K, dist, np.eye(3), K, 80, 60)
    ux, uy = undistort_map(K[0, 0], K[1, 1], K[0, 2], K[1, 2], *dist, 80, 60)
    assert mx.dtype == my.dtype == np.float32 and mx.shape == (60, 80)
    assert (mx.view(np.uint32) == ux.view(np.uint32)).all() and (my.view(np.uint32) == uy.view(np.uint32)).all()


def test_rectify_map_quarter_turn_about_the_optical_axis():
    """R turns the raw camera's axes into the rectified ones by 90 degrees about z: R^-1 (x, y, 1) = (y, -x, 1), so rectified
    pixel (u, v) samples raw pixel (cx + f (v - cy) / f, cy - f (u - cx) / f)."""
    from monogs_amd.stereo import rectify_map
    K = _K(20.0, 20.0, 8.0, 6.0)
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    mx, my = rectify_map(K, [0.0] * 5, R, K, 16, 12)
    u, v = np.meshgrid(np.arange(16.0), np.arange(12.0))
    assert np.abs(mx - (8.0 + (v - 6.0))).max() < 1e-5 and np.abs(my - (6.0 - (u - 8.0))).max() < 1e-5


def test_rectify_map_focal_change():
    """No distortion, no rotation, twice the focal length in the new camera: the rectified image is the raw one magnified by two
    about the principal point."""
    from monogs_amd.stereo import rectify_map
    mx, my = rectify_map(_K(20.0, 30.0, 8.0, 6.0), [0.0] * 5, np.eye(3), _K(40.0, 60.0, 8.0, 6.0), 16, 12)
    u, v = np.meshgrid(np.arange(16.0), np.arange(12.0))
    assert np.abs(mx - (8.0 + (u - 8.0) / 2.0)).max() < 1e-6 and np.abs(my - (6.0 + (v - 6.0) / 2.0)).max() < 1e-6


def test_calibration_maps_of_the_euroc_fixture():
    from monogs_amd.stereo import calibration_maps, rectify_map
    cal = FIXTURE["Calibration"]
    assert (cal["width"], cal["height"], cal["distorted"]) == (752, 480, True)
    maps = calibration_maps(cal)
    assert len(maps) == 4 and all(m.shape == (480, 752) and m.dtype == np.float32 for m in maps)
    # the rectified principal point looks along R^-1 z through the raw camera: close to the raw principal point
    c0 = cal["cam0"]
    assert abs(maps[0][252, 367] - c0["raw"]["cx"]) < 8 and abs(maps[1][252, 367] - c0["raw"]["cy"]) < 8
    assert not np.array_equal(maps[0], maps[2])
    assert calibration_maps(dict(cal, distorted=False)) is None
    again = rectify_map(np.array([[c0["raw"]["fx"], 0, c0["raw"]["cx"]], [0, c0["raw"]["fy"], c0["raw"]["cy"]], [0, 0, 1.0]]),
                        [c0["raw"][k] for k in ("k1", "k2", "p1", "p2", "k3")], np.array(c0["R"]["data"]).reshape(3, 3),
                        np.array([[c0["opt"]["fx"], 0, c0["opt"]["cx"]], [0, c0["opt"]["fy"], c0["opt"]["cy"]], [0, 0, 1.0]]), 752, 480)
    assert np.array_equal(again[0], maps[0]) and np.array_equal(again[1], maps[1])


# ---- EuRoC parser and dataset ------------------------------------------------------------------------------------------------
W, H = 40, 12
T0 = 1403636579763555584            # ns, as EuRoC names its files


def _gray(i, cam):
    return ((np.arange(H * W).reshape(H, W) * 5 + 17 * i + 101 * cam) % 256).astype(np.uint8)


def _write_euroc(folder, n=6, sensor_yaml=True):
    """n pairs 50 ms apart; ground truth at 5 ms steps starting 2 ms late, so that every image has one nearest row."""
    for cam in (0, 1):
        os.makedirs(folder / "mav0" / f"cam{cam}" / "data")
        for i in reversed(range(n)):
            Image.fromarray(_gray(i, cam)).save(folder / "mav0" / f"cam{cam}" / "data" / f"{T0 + i * 50_000_000}.png")
    if sensor_yaml:
        with open(folder / "mav0" / "cam0" / "sensor.yaml", "w") as f:
            f.write("# General sensor definitions.\nsensor_type: camera\ncomment: VI-Sensor cam0 (MT9M034)\n\n"
                    "# Sensor extrinsics wrt. the body-frame.\nT_BS:\n  cols: 4\n  rows: 4\n  data: ["
                    + ", ".join(repr(v) for row in FIXTURE["T_BS"] for v in row) + "]\n\nrate_hz: 20\nresolution: [752, 480]\n")
    os.makedirs(folder / "mav0" / "state_groundtruth_estimate0")
    s = math.sin(math.pi / 4)
    rows = []
    with open(folder / "mav0" / "state_groundtruth_estimate0" / "data.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["#timestamp", "p_RS_R_x [m]", "p_RS_R_y [m]", "p_RS_R_z [m]", "q_RS_w []", "q_RS_x []", "q_RS_y []", "q_RS_z []",
                    "v_RS_R_x [m s^-1]", "v_RS_R_y [m s^-1]", "v_RS_R_z [m s^-1]"])
        for k in range(n * 10 + 5):
            t = T0 + 2_000_000 + k * 5_000_000
            row = [t, 0.01 * k, -0.2, 0.3 + 0.001 * k, s, 0.0, 0.0, s, 0.0, 0.0, 0.0]         # q wxyz: 90 degrees about z
            rows.append(row)
            w.writerow(row)
    return rows


def test_euroc_parser_association_start_idx_and_quaternion_order(tmp_path):
    from monogs_amd.stereo import EuRoCParser
    rows = _write_euroc(tmp_path)
    p = EuRoCParser(str(tmp_path))
    assert p.n_img == 6 and len(p.color_paths_r) == 6 and len(p.poses) == 6
    assert [os.path.basename(c) for c in p.color_paths] == [f"{T0 + i * 50_000_000}.png" for i in range(6)]
    assert [os.path.basename(c) for c in p.color_paths_r] == [os.path.basename(c) for c in p.color_paths]
    assert "cam0" in p.color_paths[0] and "cam1" in p.color_paths_r[0]
    # image i at T0 + 50 i ms; rows at T0 + 2 + 5 k ms: the nearest is k = 10 i (2 ms away; k = 10 i - 1 is 3 ms away)
    assert p.pose_indices == [10 * i for i in range(6)]
    T_BS = np.array(FIXTURE["T_BS"])
    assert np.array_equal(p.T_i_c0, T_BS)                     # read back from the sensor.yaml written above
    # (w, x, y, z) = (cos 45, 0, 0, sin 45): 90 degrees about z, x -> y.  Taken as (x, y, z, w) it would be about x.
    for i in (0, 3):
        k = 10 * i
        T_w_i = np.array([[0.0, -1.0, 0.0, rows[k][1]], [1.0, 0.0, 0.0, rows[k][2]], [0.0, 0.0, 1.0, rows[k][3]], [0.0, 0.0, 0.0, 1.0]])
        assert p.poses[i].dtype == np.float64 and np.abs(p.poses[i] - np.linalg.inv(T_w_i @ T_BS)).max() < 1e-9
    q = EuRoCParser(str(tmp_path), start_idx=4)
    assert q.n_img == 2 and q.pose_indices == [40, 50]
    assert os.path.basename(q.color_paths[0]) == os.path.basename(q.color_paths_r[0]) == f"{T0 + 4 * 50_000_000}.png"
    assert np.array_equal(q.poses[1], p.poses[5])


def test_euroc_parser_takes_T_BS_from_the_config_and_checks_the_counts(tmp_path):
    from monogs_amd.stereo import EuRoCParser, load_stereo_dataset
    _write_euroc(tmp_path, sensor_yaml=False)
    with pytest.raises(FileNotFoundError):
        EuRoCParser(str(tmp_path))
    shift = np.eye(4)
    shift[:3, 3] = (1.0, 2.0, 3.0)
    for form in (shift.tolist(), shift.reshape(-1).tolist(), dict(rows=4, cols=4, data=shift.reshape(-1).tolist())):
        p = EuRoCParser(str(tmp_path), t_bs=form)
        assert np.array_equal(p.T_i_c0, shift)
    # world-to-camera of T_w_i shift: the camera centre is the body position plus the rotated offset (-2, 1, 3)
    centre = np.linalg.inv(p.poses[0])[:3, 3]
    assert np.abs(centre - (0.0 - 2.0, -0.2 + 1.0, 0.3 + 3.0)).max() < 1e-9
    cal = dict(FIXTURE["Calibration"], width=W, height=H, distorted=False)
    cal["cam0"] = dict(cal["cam0"], T_BS=shift.tolist())
    ds = load_stereo_dataset(dict(Dataset=dict(type="euroc", sensor_type="stereo", dataset_path=str(tmp_path), start_idx=1,
                                               Calibration=cal, Stereo=dict(num_disparities=16))), device="cpu")
    assert len(ds) == 5 and np.array_equal(ds.poses[0], p.poses[1])
    os.remove(sorted((tmp_path / "mav0" / "cam1" / "data").iterdir())[0])
    with pytest.raises(ValueError, match="cam1"):
        EuRoCParser(str(tmp_path), t_bs=shift)


def _config(folder, **stereo):
    cal = dict(FIXTURE["Calibration"], width=W, height=H, distorted=False)
    ds = dict(type="euroc", sensor_type="stereo", dataset_path=str(folder), start_idx=0, Calibration=cal)
    if stereo:
        ds["Stereo"] = stereo
    return dict(Dataset=ds)


def test_load_dataset_still_refuses_euroc_and_stereo_enters_through_its_own_loader(tmp_path):
    from monogs_amd.dataset import load_dataset
    from monogs_amd.stereo import load_stereo_dataset
    _write_euroc(tmp_path)
    with pytest.raises(ValueError, match="Unknown dataset type"):
        load_dataset(_config(tmp_path), device="cpu")
    with pytest.raises(ValueError, match="Unknown stereo dataset type"):
        load_stereo_dataset(dict(Dataset=dict(type="tum", dataset_path=str(tmp_path), Calibration={})), device="cpu")
    ds = load_stereo_dataset(_config(tmp_path, num_disparities=16), device="cpu")
    opt = FIXTURE["Calibration"]["cam0"]["opt"]
    assert (ds.fx, ds.fy, ds.cx, ds.cy) == (opt["fx"], opt["fy"], opt["cx"], opt["cy"])
    assert (ds.width, ds.height, ds.with_depth, len(ds)) == (W, H, True, 6)
    assert ds.ingest.matcher.num_disparities == 16 and ds.ingest.matcher.bf == FIXTURE["bf"] and ds.ingest.host_maps is None
    left, right = ds._decode(2)
    assert left.dtype == np.uint8 and (left == _gray(2, 0)).all() and (right == _gray(2, 1)).all()
    with pytest.raises(RuntimeError, match="no CPU path"):       # everything up to the library ran
        ds[0]
    with pytest.raises(ValueError, match="unknown keys"):
        load_stereo_dataset(_config(tmp_path, disparities=16), device="cpu")
    with pytest.raises(ValueError, match="no valid column"):
        load_stereo_dataset(_config(tmp_path), device="cpu")     # the reference's 64 disparities on a 40-pixel image
    pre = load_stereo_dataset(_config(tmp_path, num_disparities=16), device="cpu", preload=True)
    assert pre.preload and len(pre.pairs) == 6
    wrong = _config(tmp_path, num_disparities=16)
    wrong["Dataset"]["Calibration"]["width"] = W + 2
    with pytest.raises(ValueError, match="calibration"):
        load_stereo_dataset(wrong, device="cpu")._decode(0)


def test_dataset_frames_takes_a_stereo_dataset_unchanged(tmp_path, monkeypatch):
    """With the device half replaced by the mirror on the CPU: ``dataset_frames`` reads nothing a ``StereoDataset`` lacks."""
    from monogs_amd import stereo
    from monogs_amd.dataset import dataset_frames
    _write_euroc(tmp_path)

    def prepare(self, left, right):
        left, right = stereo.validate_pair(self.width, self.height, left, right)
        out = sm.stereo(left, right, D=self.matcher.num_disparities, bf=self.matcher.bf, **self.matcher.params)
        ones = torch.ones(self.height, self.width, dtype=torch.bool)
        return dict(rgb=torch.from_numpy(out["rgb"]), depth=torch.from_numpy(out["depth"]), mask=ones, grad_mask=ones,
                    segmentation=None)
    monkeypatch.setattr(stereo.StereoIngest, "prepare", prepare)
    ds = stereo.load_stereo_dataset(_config(tmp_path, num_disparities=16), device="cpu")
    frames, intr = dataset_frames(ds, 3, device="cpu", start=1, stride=2)
    assert len(frames) == 3 and (intr.width, intr.height) == (W, H) and intr.fx == ds.fx
    assert tuple(frames[0].rgb.shape) == (3, H, W) and tuple(frames[0].depth.shape) == (H, W)
    assert (frames[1].rgb[0].numpy() == np.float32(_gray(3, 0).astype(np.float64) / 255.0)).all()
    pose = torch.from_numpy(ds.poses[3]).to(torch.float32)
    assert torch.equal(frames[1].R_gt, pose[:3, :3]) and torch.equal(frames[1].T_gt, pose[:3, 3])


def test_lazy_exports():
    import monogs_amd
    from monogs_amd import stereo
    for name in ("StereoMatcher", "StereoIngest", "EuRoCParser", "StereoDataset", "load_stereo_dataset", "rectify_map"):
        assert getattr(monogs_amd, name) is getattr(stereo, name)


def test_prepare_raises_before_touching_the_device():
    from monogs_amd.stereo import StereoIngest, StereoMatcher
    si = StereoIngest(W, H, dict(distorted=False), "cuda:0", num_disparities=16)
    g = _gray(0, 0)
    with pytest.raises(ValueError, match="uint8"):
        si.prepare(g.astype(np.float32), g)
    with pytest.raises(ValueError, match="right must be"):
        si.prepare(g, g[:, :-1])
    with pytest.raises(ValueError, match="left must be"):
        si.prepare(np.dstack([g, g, g]), g)
    with pytest.raises(ValueError, match="16, 32, 48 or 64"):
        StereoMatcher(W, H, "cuda:0", num_disparities=24)
    with pytest.raises(ValueError, match="no valid column"):
        StereoMatcher(64, H, "cuda:0")


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    for s in ("mgs_stereo_scratch_bytes", "mgs_stereo_depth"):
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES and hasattr(native_lib, s)
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 18
    assert native_lib.mgs_abi_version() == _lib.ABI_VERSION
    block = text[text.index("(ABI v18)"):]
    assert "UNPINNED" in block and "125 685" in block and "= 12" in block
    assert float(re.search(r"#define MGS_EUROC_BF (\S+)", text).group(1)) == FIXTURE["bf"]
    # nine int32 (+ 4 bytes of padding), a double, thirteen pointers
    assert C.sizeof(_lib.MgsStereo) == 40 + 8 + 13 * 8
    # the scratch size the header quotes
    quoted = int(re.search(r"([\d ]+) bytes at 752 x 480 x 64", block).group(1).replace(" ", ""))
    assert native_lib.mgs_stereo_scratch_bytes(752, 480, 64) == quoted


def test_stereo_scratch_is_pure_and_monotone(native_lib):
    f = native_lib.mgs_stereo_scratch_bytes
    assert f(752, 480, 64) == f(752, 480, 64) >= 2 * 4 * 688 * 480 * 64
    for w in range(65, 140):                        # monotone in every argument, multiple of 16
        assert f(w, 7, 64) <= f(w + 1, 7, 64) and f(99, w - 64, 32) <= f(99, w - 63, 32) and f(w, 7, 64) % 16 == 0
        assert f(w, 7, 16) <= f(w, 7, 32) <= f(w, 7, 48) <= f(w, 7, 64)
    assert f(64, 7, 64) == f(100, 0, 64) == f(100, 7, 24) == 256      # sizes the entry point refuses


def _params(lib_mod, **kw):
    p = lib_mod.MgsStereo()
    p.width, p.height, p.num_disparities, p.block_size, p.uniqueness_ratio, p.bf = 100, 20, 64, 20, 40, FIXTURE["bf"]
    for k in ("left_u8", "right_u8", "rgb_out", "disp16_out", "depth_out", "scratch"):
        setattr(p, k, PTR)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_stereo_depth_refuses_bad_arguments_before_any_launch(native_lib):
    """Every refusal returns 1 with a message; nothing is launched (this runs without a device, and the pointers are never
    dereferenced)."""
    from monogs_amd import _lib
    sd = lambda **kw: native_lib.mgs_stereo_depth(C.byref(_params(_lib, **kw)), None)     # noqa: E731
    assert native_lib.mgs_stereo_depth(None, None) == 1 and "params" in _err(native_lib)
    for k in ("left_u8", "right_u8", "rgb_out", "disp16_out", "depth_out", "scratch"):
        assert sd(**{k: None}) == 1 and "non-NULL" in _err(native_lib), k
    for d in (0, 8, 24, 65, 80, 128, -16):
        assert sd(num_disparities=d) == 1 and "num_disparities" in _err(native_lib), d
    assert sd(width=64) == 1 and "width > num_disparities" in _err(native_lib)
    assert sd(height=0) == 1 and "height >= 1" in _err(native_lib)
    assert sd(width=1 << 20, height=1 << 10) == 1 and "2^31" in _err(native_lib)
    for maps in (("map_lx",), ("map_lx", "map_ly"), ("map_ly", "map_rx", "map_ry")):
        assert sd(**{k: PTR for k in maps}) == 1 and "all or none" in _err(native_lib), maps
    assert sd(block_size=64) == 1 and "block_size" in _err(native_lib)
    assert sd(p1=(1 << 20) + 1) == 1 and "p1 and p2" in _err(native_lib)
    assert sd(p2=(1 << 20) + 1) == 1 and "p1 and p2" in _err(native_lib)
    assert sd(uniqueness_ratio=101) == 1 and "uniqueness_ratio" in _err(native_lib)
    assert sd(pre_filter_cap=128) == 1 and "pre_filter_cap" in _err(native_lib)
    for bad in (float("inf"), float("nan")):
        assert sd(bf=bad) == 1 and "bf" in _err(native_lib), bad
    assert sd(scratch=PTR + 4) == 1 and "aligned" in _err(native_lib)
    assert sd(sum_out=PTR + 2) == 1 and "sum_out" in _err(native_lib)
