"""Stereo input: the EuRoC reader and the per-frame depth producer, semi-global matching in HIP.

In the reference stereo is not a different SLAM: ``StereoDataset.__getitem__`` (/root/reference/utils/dataset.py:511-629)
rectifies both grey images with ``cv2.remap``, runs ``cv2.StereoSGBM`` on the CPU (64 disparities, block 20, uniqueness 40), turns
the disparity into metric depth with a fixed ``baseline x fx`` and hands the tracker an RGB-D frame.  Here the host uploads the
two decoded 8-bit images and ``mgs_stereo_depth`` (csrc/stereo.hip) does all of that in twelve launches; ``mgs_grad_mask`` adds
its eight for the gradient mask, and the frame that comes out is what ``FrameIngest.prepare`` returns for an RGB-D one.

cv2 is not available to this project.  ``rectify_map`` restates ``cv2.initUndistortRectifyMap``, the kernels restate an 8-bit
``cv2.remap(INTER_LINEAR)`` and ``StereoSGBM`` in mode ``MODE_SGBM`` from their documented behaviour; the step-by-step
specification in include/monogs_raster.h is normative and parity with cv2 is unpinned (the kernels are bit-exact against an
integer mirror, tests/stereo_mirror.py).  One known difference is deliberate: OpenCV keeps its cost volume in 16 bits, which
wraps at the reference's block size (21 x 21 x 285 = 125 685); this one is 32-bit and does not.
"""
from __future__ import annotations

import csv
import ctypes as C
import glob
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .dataset import load_config, quaternion_pose
from .frame_ingest import _host_array, grad_mask, grad_mask_scratch
from ._launch import _device_guard, _stream

EUROC_BF = 47.90639384423901      # baseline x fx of the rectified EuRoC pair (dataset.py:610, "following ORB-SLAM2")
MATCHER_KEYS = ("num_disparities", "block_size", "uniqueness_ratio", "p1", "p2", "disp12_max_diff", "pre_filter_cap", "bf")


def rectify_map(K_raw, dist, R, K_new, width, height) -> Tuple[np.ndarray, np.ndarray]:
    """``(map_x, map_y)``, float32 ``[height, width]``: for every pixel (u, v) of the rectified image, where to sample the raw
    one -- ``initUndistortRectifyMap(K_raw, dist, R, K_new)`` in float64: the ray ``R^-1 K_new^-1 (u, v, 1)``, divided by its
    third component, through the ``k1 k2 p1 p2 k3`` model and ``K_raw``.  With ``R = I`` and ``K_new = K_raw`` it equals
    ``frame_ingest.undistort_map`` bit for bit."""
    K_raw, K_new = np.asarray(K_raw, dtype=np.float64).reshape(3, 3), np.asarray(K_new, dtype=np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3 = (float(v) for v in dist)
    Ri = np.linalg.inv(np.asarray(R, dtype=np.float64).reshape(3, 3))
    u, v = np.meshgrid(np.arange(int(width), dtype=np.float64), np.arange(int(height), dtype=np.float64))
    xn, yn = (u - K_new[0, 2]) / K_new[0, 0], (v - K_new[1, 2]) / K_new[1, 1]
    X = Ri[0, 0] * xn + Ri[0, 1] * yn + Ri[0, 2]
    Y = Ri[1, 0] * xn + Ri[1, 1] * yn + Ri[1, 2]
    Z = Ri[2, 0] * xn + Ri[2, 1] * yn + Ri[2, 2]
    x, y = X / Z, Y / Z
    r2 = x * x + y * y
    kr = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * kr + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * kr + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return (K_raw[0, 0] * xd + K_raw[0, 2]).astype(np.float32), (K_raw[1, 1] * yd + K_raw[1, 2]).astype(np.float32)


def _K(c: dict) -> np.ndarray:
    return np.array([[float(c["fx"]), 0.0, float(c["cx"])], [0.0, float(c["fy"]), float(c["cy"])], [0.0, 0.0, 1.0]])


def calibration_maps(calibration: dict):
    """The four rectification maps ``(left x, left y, right x, right y)`` of a reference-style stereo calibration
    (``cam0`` / ``cam1``: ``{raw, opt, R}``, dataset.py:574-593), or None when it is not ``distorted``."""
    if not bool(calibration.get("distorted", False)):
        return None
    W, H = int(calibration["width"]), int(calibration["height"])
    maps = []
    for cam in ("cam0", "cam1"):
        c = calibration[cam]
        maps += rectify_map(_K(c["raw"]), [c["raw"][k] for k in ("k1", "k2", "p1", "p2", "k3")],
                            np.asarray(c["R"]["data"], dtype=np.float64).reshape(3, 3), _K(c["opt"]), W, H)
    return tuple(maps)


class StereoMatcher:
    """``mgs_stereo_depth`` for one image size: owns the scratch.  The defaults are the reference's matcher
    (``StereoSGBM_create(minDisparity=0, numDisparities=64, blockSize=20)``, ``setUniquenessRatio(40)``); a parameter left at 0
    takes OpenCV's default (p1 2, p2 5, disp12_max_diff 1, pre-filter cap 15).  Nothing touches the device before the first
    ``compute``; parameters the library refuses raise there, before anything is launched."""

    def __init__(self, width: int, height: int, device, num_disparities: int = 64, block_size: int = 20,
                 uniqueness_ratio: int = 40, p1: int = 0, p2: int = 0, disp12_max_diff: int = 0, pre_filter_cap: int = 0,
                 bf: float = EUROC_BF):
        self.width, self.height, self.device = int(width), int(height), torch.device(device)
        self.num_disparities = int(num_disparities)
        if self.num_disparities not in (16, 32, 48, 64):
            raise ValueError(f"num_disparities must be 16, 32, 48 or 64 (got {num_disparities})")
        if self.height < 1 or self.width <= self.num_disparities:
            raise ValueError(f"a {self.width} x {self.height} image leaves no valid column for {self.num_disparities} disparities")
        self.params = dict(block_size=int(block_size), p1=int(p1), p2=int(p2), uniqueness_ratio=int(uniqueness_ratio),
                           disp12_max_diff=int(disp12_max_diff), pre_filter_cap=int(pre_filter_cap))
        self.bf = float(bf)
        self.scratch = None

    def scratch_bytes(self) -> int:
        return int(_lib.load().mgs_stereo_scratch_bytes(self.width, self.height, self.num_disparities))

    @torch.no_grad()
    def compute(self, left_u8: torch.Tensor, right_u8: torch.Tensor, maps: Optional[Sequence[torch.Tensor]] = None,
                debug: Optional[dict] = None, scratch: Optional[torch.Tensor] = None):
        """``(disp16, depth, rgb)`` of a pair of uint8 ``[H, W]`` device images, on the current stream: int16 ``[H, W]``
        disparities in sixteenths (-16: invalid), float32 ``[H, W]`` depth = bf / disparity (0 where invalid), float32
        ``[3, H, W]`` grey left image.  ``maps``: four float32 ``[H, W]`` device maps (left x, left y, right x, right y) to
        rectify through.  Twelve launches, no host synchronisation, capturable.  A ``debug`` dict is filled with ``rect_l``,
        ``rect_r`` (uint8) and ``S`` (int32 ``[H, W - D, D]``, the aggregated cost volume)."""
        H, W, D, dev = self.height, self.width, self.num_disparities, self.device
        if dev.type != "cuda":
            raise RuntimeError("StereoMatcher: no CPU path (the stereo kernels are HIP only)")
        for t, what in ((left_u8, "left_u8"), (right_u8, "right_u8")):
            if not torch.is_tensor(t) or t.device != dev or t.dtype != torch.uint8 or tuple(t.shape) != (H, W) or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous uint8 tensor of shape [{H}, {W}] on {dev}")
        if maps is not None:
            if len(maps) != 4:
                raise ValueError("maps: four tensors (left x, left y, right x, right y)")
            for m in maps:
                if m.device != dev or m.dtype != torch.float32 or tuple(m.shape) != (H, W) or not m.is_contiguous():
                    raise ValueError(f"every map must be a contiguous float32 tensor of shape [{H}, {W}] on {dev}")
        lib = _lib.load()
        if scratch is None:
            if self.scratch is None:
                self.scratch = torch.empty(self.scratch_bytes(), dtype=torch.uint8, device=dev)
            scratch = self.scratch
        p = _lib.MgsStereo()
        p.width, p.height, p.num_disparities = W, H, D
        for k, v in self.params.items():
            setattr(p, k, v)
        p.bf = self.bf
        p.left_u8, p.right_u8 = left_u8.data_ptr(), right_u8.data_ptr()
        if maps is not None:
            p.map_lx, p.map_ly, p.map_rx, p.map_ry = (m.data_ptr() for m in maps)
        rgb = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        disp16 = torch.empty(H, W, dtype=torch.int16, device=dev)
        depth = torch.empty(H, W, dtype=torch.float32, device=dev)
        p.rgb_out, p.disp16_out, p.depth_out = rgb.data_ptr(), disp16.data_ptr(), depth.data_ptr()
        if debug is not None:
            debug["rect_l"] = torch.empty(H, W, dtype=torch.uint8, device=dev)
            debug["rect_r"] = torch.empty(H, W, dtype=torch.uint8, device=dev)
            debug["S"] = torch.empty(H, W - D, D, dtype=torch.int32, device=dev)
            p.left_rect_out, p.right_rect_out, p.sum_out = (debug[k].data_ptr() for k in ("rect_l", "rect_r", "S"))
        p.scratch = scratch.data_ptr()
        with _device_guard(dev):
            _lib.check(lib.mgs_stereo_depth(C.byref(p), _stream()), "mgs_stereo_depth")
        return disp16, depth, rgb


def validate_pair(width: int, height: int, left, right):
    """The host-side checks of ``StereoIngest.prepare``; touches no device.  Returns two C-contiguous uint8 ``[H, W]`` arrays."""
    out = []
    for a, what in ((left, "left"), (right, "right")):
        a = _host_array(a, what)
        if a.dtype != np.uint8:
            raise ValueError(f"{what} must be uint8 (got {a.dtype})")
        if a.shape != (height, width):
            raise ValueError(f"{what} must be a grey image of shape [{height}, {width}] (got {list(a.shape)})")
        out.append(np.ascontiguousarray(a))
    return out


class StereoIngest:
    """The stereo sibling of ``FrameIngest``: the device half of the dataset for one image size.  Owns the four rectification
    maps (when ``calibration["distorted"]``), the matcher and its scratch, the scratch of ``mgs_grad_mask`` and one pair's
    pinned staging and device input buffers.  ``matcher``: keyword arguments of ``StereoMatcher``."""

    def __init__(self, width: int, height: int, calibration: dict, device, **matcher):
        self.width, self.height, self.device = int(width), int(height), torch.device(device)
        if self.width < 2 or self.height < 2:
            raise ValueError("StereoIngest needs an image of at least 2 x 2 pixels")        # (the gradient mask's reflect padding)
        self.host_maps = calibration_maps(dict(calibration, width=self.width, height=self.height))
        self.matcher = StereoMatcher(self.width, self.height, self.device, **matcher)
        self._ready = False

    def _allocate(self):
        H, W, dev = self.height, self.width, self.device
        if dev.type != "cuda":
            raise RuntimeError("StereoIngest: no CPU path (the stereo kernels are HIP only)")
        self.maps = None if self.host_maps is None else tuple(torch.from_numpy(m).to(dev) for m in self.host_maps)
        self.grad_scratch = grad_mask_scratch(W, H, dev)
        self._pin = [torch.empty(H, W, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._in = [torch.empty(H, W, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._uploaded = torch.cuda.Event()
        self._ready = True

    @torch.no_grad()
    def prepare_device(self, left_u8: torch.Tensor, right_u8: torch.Tensor) -> Dict[str, Optional[torch.Tensor]]:
        """``mgs_stereo_depth`` and ``mgs_grad_mask`` on device images, on the current stream: twenty launches (and torch's fill of the
        all-ones mask) into fresh outputs, no host synchronisation, capturable."""
        if not self._ready:
            self._allocate()
        disp16, depth, rgb = self.matcher.compute(left_u8, right_u8, self.maps)
        return dict(rgb=rgb, depth=depth, mask=torch.ones(self.height, self.width, dtype=torch.bool, device=self.device),
                    grad_mask=grad_mask(rgb, scratch=self.grad_scratch), disp16=disp16)

    def prepare(self, left, right) -> Dict[str, Optional[torch.Tensor]]:
        """One decoded pair (numpy arrays or CPU tensors, uint8 [H,W]) -> the dict ``FrameIngest.prepare`` returns for an RGB-D
        frame: ``rgb`` float32 [3,H,W] (the rectified left image on all three channels), ``depth`` float32 [H,W], ``mask`` bool
        (all ones, as without a segmentation), ``segmentation`` None, ``grad_mask`` bool; plus ``disp16``.  A wrong dtype or
        shape raises ``ValueError`` before the device is touched."""
        pair = validate_pair(self.width, self.height, left, right)
        if not self._ready:
            self._allocate()
        with _device_guard(self.device):
            self._uploaded.synchronize()                  # the previous pair's copies have left the pinned buffers
            for k in range(2):
                self._pin[k].numpy()[...] = pair[k]
                self._in[k].copy_(self._pin[k], non_blocking=True)
            self._uploaded.record()
            out = self.prepare_device(self._in[0], self._in[1])
        out["segmentation"] = None
        return out


# ---- EuRoC -------------------------------------------------------------------------------------------------------------------
def _matrix4(v) -> np.ndarray:
    """A 4x4 from a YAML value: ``{rows, cols, data: [16]}``, a flat list of 16 or four rows of four."""
    if isinstance(v, dict):
        v = v["data"]
    return np.asarray(v, dtype=np.float64).reshape(4, 4)


def read_T_BS(sensor_yaml: str) -> np.ndarray:
    """``T_BS`` (sensor to body) of an EuRoC ``sensor.yaml``."""
    import yaml
    with open(sensor_yaml, "r", encoding="utf-8") as f:
        text = "".join(ln for ln in f if not ln.startswith("%"))          # (an OpenCV-style "%YAML:1.0" first line is not YAML)
    return _matrix4(yaml.safe_load(text)["T_BS"])


class EuRoCParser:
    """``mav0/cam0/data/*.png`` and ``mav0/cam1/data/*.png`` (sorted, equal counts, both from ``start_idx``) and
    ``mav0/state_groundtruth_estimate0/data.csv`` (a header row, then t, p xyz, q wxyz, ...).  Each image takes the ground-truth
    row nearest in time to its file-name stem; ``poses[i] = inv(T_w_i T_i_c0)``, world-to-camera, with ``T_i_c0`` the ``T_BS`` of
    ``mav0/cam0/sensor.yaml`` unless ``t_bs`` (the config key ``Dataset.Calibration.cam0.T_BS``) is given."""

    def __init__(self, folder: str, start_idx: int = 0, t_bs=None):
        self.input_folder, self.start_idx = folder, int(start_idx)
        left = sorted(glob.glob(os.path.join(folder, "mav0", "cam0", "data", "*.png")))
        right = sorted(glob.glob(os.path.join(folder, "mav0", "cam1", "data", "*.png")))
        if len(left) != len(right):
            raise ValueError(f"{folder}: {len(left)} cam0 images and {len(right)} cam1 images")
        self.color_paths, self.color_paths_r = left[self.start_idx:], right[self.start_idx:]
        self.n_img = len(self.color_paths)
        self.T_i_c0 = _matrix4(t_bs) if t_bs is not None else read_T_BS(os.path.join(folder, "mav0", "cam0", "sensor.yaml"))
        with open(os.path.join(folder, "mav0", "state_groundtruth_estimate0", "data.csv"), "r", encoding="utf-8", newline="") as f:
            reader = csv.reader(f)
            next(reader)                                   # the header row
            data = np.array([[float(v) for v in row] for row in reader if row], dtype=np.float64)
        self.timestamps = [float(os.path.splitext(os.path.basename(p))[0]) for p in self.color_paths]
        self.pose_indices = [int(np.argmin(np.abs(data[:, 0] - t))) for t in self.timestamps]
        self.poses = []
        for k in self.pose_indices:
            q_wxyz = data[k, 4:8]
            T_w_i = quaternion_pose(data[k, 1:4], q_wxyz[[1, 2, 3, 0]])
            self.poses.append(np.linalg.inv(T_w_i @ self.T_i_c0))


class StereoDataset:
    """The reference's ``StereoDataset`` over an ``EuRoCParser``: ``dataset[i]`` decodes pair ``i`` with PIL (as 8-bit grey) and
    hands it to ``StereoIngest.prepare``; returns that dict plus ``pose`` (float64 [4,4] world-to-camera).  Calibration keys as
    in the reference: ``cam0`` / ``cam1`` ``{raw, opt, R}``, ``distorted``, ``width``, ``height``; the intrinsics the tracker
    sees are ``cam0.opt``.  ``Dataset.Stereo`` (this project's key, optional) overrides matcher arguments by name
    (``num_disparities``, ``block_size``, ``uniqueness_ratio``, ``p1``, ``p2``, ``disp12_max_diff``, ``pre_filter_cap``,
    ``bf``); without it the reference's fixed matcher runs."""

    with_depth = True

    def __init__(self, parser, config: dict, device="cuda:0", preload: bool = False):
        cal = config["Dataset"]["Calibration"]
        self.calibration = dict(cal)
        self.device = device
        opt = cal["cam0"]["opt"]
        self.fx, self.fy, self.cx, self.cy = (float(opt[k]) for k in ("fx", "fy", "cx", "cy"))
        self.width, self.height = int(cal["width"]), int(cal["height"])
        self.K = _K(opt)
        self.distorted = bool(cal["distorted"])
        self.color_paths, self.color_paths_r, self.poses = parser.color_paths, parser.color_paths_r, parser.poses
        self.num_imgs = len(self.color_paths)
        matcher = dict(config["Dataset"].get("Stereo") or {})
        unknown = sorted(set(matcher) - set(MATCHER_KEYS))
        if unknown:
            raise ValueError(f"Dataset.Stereo: unknown keys {unknown}")
        self.ingest = StereoIngest(self.width, self.height, self.calibration, device, **matcher)
        self.preload = False
        self.pairs = []
        if preload:
            self.load_data()

    def __len__(self):
        return self.num_imgs

    def _decode(self, idx: int):
        from PIL import Image
        pair = []
        for p in (self.color_paths[idx], self.color_paths_r[idx]):
            im = Image.open(p)
            a = np.array(im if im.mode == "L" else im.convert("L"))
            if a.shape != (self.height, self.width):
                raise ValueError(f"{p}: {a.shape[1]} x {a.shape[0]} pixels, the calibration says {self.width} x {self.height}")
            pair.append(a)
        return pair

    def load_data(self):
        """Decode every pair up front; the device work stays per ``__getitem__``."""
        self.pairs = [self._decode(i) for i in range(self.num_imgs)]
        self.preload = True

    def __getitem__(self, idx: int) -> Dict[str, Optional[torch.Tensor]]:
        if not 0 <= idx < self.num_imgs:
            raise IndexError(idx)
        left, right = self.pairs[idx] if self.preload else self._decode(idx)
        data = self.ingest.prepare(left, right)
        data["pose"] = torch.from_numpy(np.asarray(self.poses[idx], dtype=np.float64)).to(self.device)
        return data


def load_stereo_dataset(config, device="cuda:0", preload: bool = False) -> StereoDataset:
    """``config``: a path to a YAML or a dict with ``Dataset: {type: euroc, sensor_type: stereo, dataset_path, start_idx,
    Calibration: {cam0, cam1, distorted, width, height}}`` -- the reference's keys (configs/stereo/euroc).  The only way in for
    stereo: ``dataset.load_dataset`` keeps refusing ``euroc``."""
    config = load_config(config)
    ds = config["Dataset"]
    if ds.get("type") != "euroc":
        raise ValueError("Unknown stereo dataset type")
    t_bs = (ds["Calibration"].get("cam0") or {}).get("T_BS")
    parser = EuRoCParser(ds["dataset_path"], start_idx=int(ds.get("start_idx") or 0), t_bs=t_bs)
    return StereoDataset(parser, config, device=device, preload=preload)
