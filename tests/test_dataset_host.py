"""The dataset readers and the host half of the frame ingest without a GPU: the TUM / Replica parsers on directories written
here, ``load_config``'s inheritance, ``undistort_map`` against the mirror (tests/ingest_mirror.py), the C ABI's argument
refusals (nothing is launched), the scratch size and ``FrameIngest.prepare``'s host-side checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import ingest_mirror as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mgs_grad_mask_scratch_bytes", "mgs_grad_mask", "mgs_frame_prepare")
PTR = 0x1000                          # non-NULL, 16-byte aligned and never dereferenced
W, H = 8, 6
FR1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628,
           k3=1.163314)


def _err(lib):
    return lib.mgs_last_error().decode()


def _colour(i):
    return ((np.arange(H * W * 3).reshape(H, W, 3) * 7 + 31 * i) % 256).astype(np.uint8)


def _depth(i):
    return ((np.arange(H * W).reshape(H, W) * 991 + 4099 * i) % 65536).astype(np.uint16)


def _calibration(**kw):
    cal = dict(fx=6.0, fy=6.5, cx=3.5, cy=2.5, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, distorted=False, width=W, height=H,
               depth_scale=5000.0, use_depth=True)
    cal.update(kw)
    return cal


# ---- TUM ---------------------------------------------------------------------------------------------------------------------
def _write_tum(folder, t_rgb, t_depth, poses, pose_file="groundtruth.txt", image_size=(W, H)):
    """``poses``: rows (t, tx, ty, tz, qx, qy, qz, qw)."""
    os.makedirs(folder / "rgb"), os.makedirs(folder / "depth")
    with open(folder / "rgb.txt", "w") as f:
        f.write("# color images\n# file: 'test'\n# timestamp filename\n")
        for i, t in enumerate(t_rgb):
            a = _colour(i)
            if image_size != (W, H):
                a = np.zeros((image_size[1], image_size[0], 3), dtype=np.uint8)
            Image.fromarray(a).save(folder / "rgb" / f"{t:.6f}.png")
            f.write(f"{t:.6f} rgb/{t:.6f}.png\n")
    with open(folder / "depth.txt", "w") as f:
        f.write("# depth maps\n# file: 'test'\n# timestamp filename\n")
        for i, t in enumerate(t_depth):
            Image.fromarray(_depth(i)).save(folder / "depth" / f"{t:.6f}.png")
            f.write(f"{t:.6f} depth/{t:.6f}.png\n")
    with open(folder / pose_file, "w") as f:
        f.write("# ground truth trajectory\n# file: 'test'\n# timestamp tx ty tz qx qy qz qw\n")
        for row in poses:
            f.write(" ".join(f"{v:.9f}" for v in row) + "\n")


def _tum_case(tmp_path, pose_file="groundtruth.txt"):
    # ten colour frames 0.04 s apart; frame 3 has a twin 0.02 s later (dropped: less than 1/32 s after the kept one);
    # the depth list has a hole around t = 0.32 (frame 8): its nearest depth is 0.081 s away
    t_rgb = [1.00, 1.04, 1.08, 1.12, 1.14, 1.16, 1.20, 1.24, 1.32, 1.40]
    t_depth = [1.001, 1.041, 1.081, 1.121, 1.161, 1.201, 1.239, 1.401]
    s = math.sin(math.pi / 4)
    poses = [(t, 0.1 * i, -0.2, 0.3 + 0.01 * i, 0.0, 0.0, s, s) for i, t in enumerate(t_rgb)]
    _write_tum(tmp_path, t_rgb, t_depth, poses, pose_file)
    return t_rgb, t_depth, poses


def test_tum_association_and_subsampling(tmp_path):
    from monogs_amd.dataset import TUMParser
    t_rgb, t_depth, _ = _tum_case(tmp_path)
    p = TUMParser(str(tmp_path))
    # 1.14 is dropped (0.02 s after 1.12), 1.32 is dropped (nearest depth 1.239 or 1.401: 0.081 s away)
    assert abs(min(abs(t - 1.32) for t in t_depth) - 0.081) < 1e-9
    kept = [1.00, 1.04, 1.08, 1.12, 1.16, 1.20, 1.24, 1.40]
    assert p.n_img == len(kept) and p.timestamps == kept
    assert [os.path.basename(c) for c in p.color_paths] == [f"{t:.6f}.png" for t in kept]
    assert [os.path.basename(d) for d in p.depth_paths] == [f"{t:.6f}.png" for t in (1.001, 1.041, 1.081, 1.121, 1.161, 1.201, 1.239, 1.401)]
    assert all(os.path.isfile(c) for c in p.color_paths + p.depth_paths)        # ('#' headers were not taken for rows)


def test_tum_pose_is_the_inverse_of_the_listed_camera_to_world(tmp_path):
    from monogs_amd.dataset import TUMParser
    _tum_case(tmp_path)
    p = TUMParser(str(tmp_path))
    # (qx, qy, qz, qw) = (0, 0, sin 45, cos 45): 90 degrees about z, x -> y.  Had the order been taken as (qw, qx, qy, qz) the
    # rotation would be about y.
    c2w = np.array([[0.0, -1.0, 0.0, 0.1], [1.0, 0.0, 0.0, -0.2], [0.0, 0.0, 1.0, 0.31], [0.0, 0.0, 0.0, 1.0]])
    assert p.poses[1].dtype == np.float64 and p.poses[1].shape == (4, 4)
    assert np.abs(p.poses[1] - np.linalg.inv(c2w)).max() < 1e-8
    assert np.abs(p.poses[1] @ c2w - np.eye(4)).max() < 1e-8


def test_tum_pose_txt_is_the_fallback(tmp_path):
    from monogs_amd.dataset import TUMParser
    _tum_case(tmp_path, pose_file="pose.txt")
    assert TUMParser(str(tmp_path)).n_img == 8
    os.remove(tmp_path / "pose.txt")
    with pytest.raises(FileNotFoundError):
        TUMParser(str(tmp_path))


# ---- Replica -----------------------------------------------------------------------------------------------------------------
def _write_replica(folder, n=10):
    os.makedirs(folder / "results")
    mats = []
    for i in reversed(range(n)):                       # written in reverse: the pairing must come from sorting
        Image.fromarray(_colour(i)).save(folder / "results" / f"frame{i:06d}.jpg", quality=95)
        Image.fromarray(_depth(i)).save(folder / "results" / f"depth{i:06d}.png")
    for i in range(n):
        a = 0.1 * i
        m = np.array([[math.cos(a), 0.0, math.sin(a), 0.5 * i], [0.0, 1.0, 0.0, -0.25], [-math.sin(a), 0.0, math.cos(a), 1.0 + i],
                      [0.0, 0.0, 0.0, 1.0]])
        mats.append(m)
    with open(folder / "traj.txt", "w") as f:
        for m in mats:
            f.write(" ".join(f"{v:.12e}" for v in m.reshape(-1)) + "\n")
    return mats


def test_replica_sorted_pairing_and_trajectory_inversion(tmp_path):
    from monogs_amd.dataset import ReplicaParser
    mats = _write_replica(tmp_path)
    p = ReplicaParser(str(tmp_path))
    assert p.n_img == 10
    assert [os.path.basename(c) for c in p.color_paths] == [f"frame{i:06d}.jpg" for i in range(10)]
    assert [os.path.basename(d) for d in p.depth_paths] == [f"depth{i:06d}.png" for i in range(10)]
    for m, pose in zip(mats, p.poses):
        assert np.abs(pose @ m - np.eye(4)).max() < 1e-9
    assert np.abs(p.poses[3][:3, 3] + mats[3][:3, :3].T @ mats[3][:3, 3]).max() < 1e-9      # t_cw = -R^T t_wc


# ---- configuration -----------------------------------------------------------------------------------------------------------
def test_load_config_follows_inherit_from_twice(tmp_path):
    from monogs_amd.dataset import load_config
    os.makedirs(tmp_path / "a" / "b")
    (tmp_path / "root.yaml").write_text("Dataset:\n  type: tum\n  Calibration:\n    fx: 1.0\n    fy: 2.0\n    distorted: False\n"
                                        "Training:\n  kf_interval: 5\n")
    (tmp_path / "a" / "mid.yaml").write_text("inherit_from: ../root.yaml\nDataset:\n  Calibration:\n    fy: 20.0\n    depth_scale: 5000.0\n")
    (tmp_path / "a" / "b" / "leaf.yaml").write_text(f"inherit_from: {tmp_path / 'a' / 'mid.yaml'}\n"
                                                    "Dataset:\n  dataset_path: somewhere\n  Calibration:\n    fx: 10.0\nResults:\n  save: True\n")
    cfg = load_config(str(tmp_path / "a" / "b" / "leaf.yaml"))
    assert cfg["Dataset"]["Calibration"] == dict(fx=10.0, fy=20.0, distorted=False, depth_scale=5000.0)   # nested override, child wins
    assert cfg["Dataset"]["type"] == "tum" and cfg["Dataset"]["dataset_path"] == "somewhere"             # keys added at every level
    assert cfg["Training"] == dict(kf_interval=5) and cfg["Results"] == dict(save=True)
    d = dict(Dataset=dict(type="tum"))
    assert load_config(d) is d


def test_unknown_dataset_type_is_refused():
    from monogs_amd.dataset import load_dataset
    with pytest.raises(ValueError, match="Unknown dataset type"):
        load_dataset(dict(Dataset=dict(type="euroc", dataset_path="x", Calibration=_calibration())), device="cpu")


def test_dataset_lengths_depth_switch_and_size_check(tmp_path):
    from monogs_amd.dataset import dataset_frames, load_dataset
    _tum_case(tmp_path / "ok")
    cfg = dict(Dataset=dict(type="tum", dataset_path=str(tmp_path / "ok"), Calibration=_calibration()))
    ds = load_dataset(cfg, device="cpu")
    assert len(ds) == 8 and ds.with_depth
    color, depth = ds._decode(2)
    assert color.dtype == np.uint8 and (color == _colour(2)).all() and (depth == _depth(2)).all()
    cfg["Dataset"]["Calibration"] = _calibration(use_depth=False)
    mono = load_dataset(cfg, device="cpu")
    assert not mono.with_depth and mono._decode(0)[1] is None
    with pytest.raises(ValueError, match="RGB-D"):
        dataset_frames(mono, 2, device="cpu")
    cfg["Dataset"]["Calibration"] = _calibration(width=W + 2)
    with pytest.raises(ValueError, match="calibration"):
        load_dataset(cfg, device="cpu")._decode(0)
    # an alpha channel is dropped
    Image.fromarray(np.dstack([_colour(0), np.full((H, W), 9, np.uint8)])).save(ds.color_paths[0])
    assert ds._decode(0)[0].shape == (H, W, 3) and (ds._decode(0)[0] == _colour(0)).all()
    pre = load_dataset(dict(Dataset=dict(type="tum", dataset_path=str(tmp_path / "ok"), Calibration=_calibration())), device="cpu", preload=True)
    assert pre.preload and len(pre.color_imgs) == len(pre.depth_imgs) == 8


# ---- undistortion map --------------------------------------------------------------------------------------------------------
def test_undistort_map_equals_the_mirror_and_is_the_identity_without_distortion():
    from monogs_amd.frame_ingest import undistort_map
    s = 1.0 / 8.0
    args = (FR1["fx"] * s, FR1["fy"] * s, FR1["cx"] * s, FR1["cy"] * s, FR1["k1"], FR1["k2"], FR1["p1"], FR1["p2"], FR1["k3"], 80, 60)
    mx, my = undistort_map(*args)
    rx, ry = im.undistort_map(*args)
    assert mx.dtype == my.dtype == np.float32 and mx.shape == my.shape == (60, 80)
    assert np.abs(mx.astype(np.float64) - rx).max() <= 1e-5 and np.abs(my.astype(np.float64) - ry).max() <= 1e-5   # one float32 ulp at 82
    outside = (mx < 0) | (mx > 79) | (my < 0) | (my > 59)
    assert 0.05 < outside.mean() < 0.12 and mx.min() < -2.9 and mx.max() > 82.0      # the GPU test's border cases exist
    ix, iy = undistort_map(6.0, 6.5, 3.5, 2.5, 0.0, 0.0, 0.0, 0.0, 0.0, 9, 7)
    u, v = np.meshgrid(np.arange(9, dtype=np.float32), np.arange(7, dtype=np.float32))
    assert (ix == u).all() and (iy == v).all()


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES and hasattr(native_lib, s)
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 16
    assert native_lib.mgs_abi_version() == _lib.ABI_VERSION
    block = text[text.index("(ABI v16)"):]
    assert "UNPINNED" in block and "NOT remapped" in block
    # int32 x 2, 5 pointers + a double, 8 words, 5 pointers, 2 floats, 1 pointer
    assert C.sizeof(_lib.MgsFramePrepare) == 8 + 4 * 8 + 8 + 8 + 32 + 5 * 8 + 8 + 8


def test_grad_mask_scratch_is_pure_and_monotone(native_lib):
    f, med = native_lib.mgs_grad_mask_scratch_bytes, native_lib.mgs_median_scratch_bytes
    sizes = [f(w, h) for w, h in ((2, 2), (5, 4), (37, 23), (80, 60), (640, 480), (1200, 680), (1920, 1080))]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert f(640, 480) == f(640, 480) == sizes[4] >= 640 * 480 * 4 + med(640 * 480)
    for w in range(2, 70):                          # monotone in either argument, multiple of 16
        assert f(w, 7) <= f(w + 1, 7) and f(7, w) <= f(7, w + 1) and f(w, 7) % 16 == 0


def _params(lib_mod, **kw):
    p = lib_mod.MgsFramePrepare()
    p.width, p.height = 8, 6
    for k in ("rgb_u8", "rgb_out", "mask_out", "grad_mask_out", "scratch"):
        setattr(p, k, PTR)
    p.edge_threshold, p.eps, p.depth_scale = 1.1, 0.01, 5000.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_frame_prepare_refuses_bad_arguments_before_any_launch(native_lib):
    """Every refusal returns 1 with a message; nothing is launched (this runs without a device, and the pointers are never
    dereferenced)."""
    from monogs_amd import _lib
    fp = lambda **kw: native_lib.mgs_frame_prepare(C.byref(_params(_lib, **kw)), None)     # noqa: E731
    assert native_lib.mgs_frame_prepare(None, None) == 1 and "params" in _err(native_lib)
    for k in ("rgb_u8", "rgb_out", "mask_out", "grad_mask_out", "scratch"):
        assert fp(**{k: None}) == 1 and "non-NULL" in _err(native_lib), k
    assert fp(map_x=PTR) == 1 and "both or neither" in _err(native_lib)
    assert fp(map_y=PTR) == 1 and "both or neither" in _err(native_lib)
    assert fp(depth_u16=PTR) == 1 and "depth_out" in _err(native_lib)
    assert fp(depth_out=PTR) == 1 and "depth_u16" in _err(native_lib)
    for bad in (0.0, -5000.0, float("inf"), float("nan")):
        assert fp(depth_u16=PTR, depth_out=PTR, depth_scale=bad) == 1 and "depth_scale" in _err(native_lib), bad
    for w, h in ((1, 6), (8, 1), (0, 0), (-4, 6)):
        assert fp(width=w, height=h) == 1 and "at least 2" in _err(native_lib), (w, h)
    assert fp(scratch=PTR + 4) == 1 and "aligned" in _err(native_lib)


def test_grad_mask_refuses_bad_arguments_before_any_launch(native_lib):
    g = native_lib.mgs_grad_mask
    assert g(1, 6, PTR, 1.1, 0.01, PTR, PTR, None, None) == 1 and "at least 2" in _err(native_lib)
    assert g(8, 1, PTR, 1.1, 0.01, PTR, PTR, None, None) == 1 and "at least 2" in _err(native_lib)
    assert g(8, 6, None, 1.1, 0.01, PTR, PTR, None, None) == 1 and "non-NULL" in _err(native_lib)
    assert g(8, 6, PTR, 1.1, 0.01, None, PTR, None, None) == 1 and "non-NULL" in _err(native_lib)
    assert g(8, 6, PTR, 1.1, 0.01, PTR, None, None, None) == 1 and "non-NULL" in _err(native_lib)
    assert g(46341, 46341, PTR, 1.1, 0.01, PTR, PTR, None, None) == 1 and "2^31" in _err(native_lib)


# ---- FrameIngest, host side --------------------------------------------------------------------------------------------------
def test_prepare_raises_before_touching_the_device():
    """`device="cuda:0"` on a machine without one: reaching the device would raise something other than ValueError."""
    from monogs_amd.frame_ingest import FrameIngest, masked_id_words, validate_frame
    fi = FrameIngest(W, H, _calibration(), "cuda:0")
    rgb, depth, seg = _colour(0), _depth(0), np.zeros((H, W), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        fi.prepare(rgb.astype(np.float32))
    with pytest.raises(ValueError, match="rgb_u8 must be"):
        fi.prepare(rgb[:, :-1])
    with pytest.raises(ValueError, match="rgb_u8 must be"):
        fi.prepare(rgb.transpose(2, 0, 1))
    with pytest.raises(ValueError, match="integer"):
        fi.prepare(rgb, depth.astype(np.float64) / 5000.0)
    with pytest.raises(ValueError, match="depth_u16 must be"):
        fi.prepare(rgb, depth[:-1])
    with pytest.raises(ValueError, match="16 bits"):
        fi.prepare(rgb, depth.astype(np.int32) + 65536)
    with pytest.raises(ValueError, match="16 bits"):
        fi.prepare(rgb, depth.astype(np.int32) - 70000)
    with pytest.raises(ValueError, match="segmentation must be uint8"):
        fi.prepare(rgb, depth, seg.astype(np.int64))
    with pytest.raises(ValueError, match="segmentation must be"):
        fi.prepare(rgb, depth, seg[:, 1:])
    with pytest.raises(ValueError, match="numpy array or a CPU tensor"):
        fi.prepare([[0]])
    with pytest.raises(ValueError, match="0..255"):
        FrameIngest(W, H, _calibration(), "cuda:0", masked_ids=(3, 256))
    with pytest.raises(ValueError, match="0..255"):
        masked_id_words([-1])
    assert masked_id_words([0, 7, 255]) == (0x81, 0, 0, 0, 0, 0, 0, 0x80000000)
    # what passes: CPU tensors and any integer depth that fits
    r, d, s = validate_frame(W, H, torch.from_numpy(rgb), depth.astype(np.int32), torch.from_numpy(seg))
    assert r.dtype == np.uint8 and d.dtype == np.uint16 and (d == depth).all() and s.dtype == np.uint8
    assert FrameIngest(80, 60, dict(FR1, distorted=True), "cuda:0").host_maps[0].shape == (60, 80)
