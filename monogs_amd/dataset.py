"""Readers for the two RGB-D layouts of BASELINE configs 3 and 4: TUM RGB-D and Replica.

What the reference's ``load_config`` (/root/reference/utils/config_utils.py:4-50), ``TUMParser`` / ``ReplicaParser``
(/root/reference/utils/dataset.py:106-207) and ``MonocularDataset`` (:305-508) do, written from their behaviour: the host
parses the lists and decodes the files with PIL, everything after the decode is ``monogs_amd.frame_ingest.FrameIngest`` on the
device.  trimesh is replaced by the quaternion formula it was used for, cv2 by ``frame_ingest.undistort_map`` and the remap
inside ``mgs_frame_prepare`` (parity with cv2 unpinned: it is not available to this project).

EuRoC stereo lives in ``monogs_amd.stereo`` (``load_stereo_dataset``: the reader and semi-global matching in HIP); ``load_dataset``
here keeps refusing ``type: euroc``.  Monocular operation (``configs/mono/*``, ``Dataset.sensor_type: monocular``):
``dataset_frames(..., monocular=True)`` builds depthless frames from any dataset -- depth files, if present, are not read -- which
``run_slam(sensor="monocular")`` tracks and maps with the RGB-only losses and ``monocular.pseudo_depth``; without the argument a
dataset that brings no depth is still refused.  What stays out: the Kubric (TIFF depth) and DAVIS (no depth) parsers and RealSense.
"""
from __future__ import annotations

import glob
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from .frame_ingest import FrameIngest
from .frames import Intrinsics, Viewpoint

MAX_DT = 0.08          # s: a colour frame needs a depth frame and a pose this close (dataset.py:148)
FRAME_RATE = 32.0      # Hz: kept colour frames are more than 1 / 32 s apart (dataset.py:138,186-191)


# ---- configuration -----------------------------------------------------------------------------------------------------------
def _merge(base: dict, child: dict) -> dict:
    """``child`` over ``base``, nested dicts key by key, in place (config_utils.py:36-50)."""
    for k, v in child.items():
        if isinstance(v, dict):
            if not isinstance(base.get(k), dict):
                base[k] = {}
            _merge(base[k], v)
        else:
            base[k] = v
    return base


def load_config(path) -> dict:
    """A YAML configuration with its ``inherit_from`` chain resolved, the including file winning.  A relative ``inherit_from``
    is tried as given (the reference is run from its repository root) and then relative to the including file.  A dict is
    returned as it is."""
    if isinstance(path, dict):
        return path
    import yaml                      # (lazily: only reading a YAML needs it)
    with open(path, "r", encoding="utf-8") as f:
        special = yaml.safe_load(f) or {}
    parent = special.get("inherit_from")
    cfg: dict = {}
    if parent is not None:
        if not os.path.isabs(parent) and not os.path.isfile(parent):
            beside = os.path.join(os.path.dirname(os.path.abspath(path)), parent)
            if os.path.isfile(beside):
                parent = beside
        cfg = load_config(parent)
    return _merge(cfg, special)


# ---- parsers -----------------------------------------------------------------------------------------------------------------
def _read_table(path: str) -> List[List[str]]:
    with open(path, "r", encoding="utf-8") as f:
        rows = [ln.split() for ln in f if ln.strip() and not ln.lstrip().startswith("#")]
    return rows


def quaternion_pose(t, q_xyzw) -> np.ndarray:
    """Camera-to-world 4x4 (float64) of a TUM pose line's ``tx ty tz`` and ``qx qy qz qw``; the quaternion is normalised."""
    x, y, z, w = np.asarray(q_xyzw, dtype=np.float64) / np.linalg.norm(np.asarray(q_xyzw, dtype=np.float64))
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = t
    return T


class TUMParser:
    """``rgb.txt`` / ``depth.txt`` / ``groundtruth.txt`` (or ``pose.txt``) of a TUM RGB-D sequence.  ``poses`` are
    world-to-camera: the inverse of the listed camera-to-world pose."""

    def __init__(self, folder: str):
        self.input_folder = folder
        pose_list = next((p for p in (os.path.join(folder, n) for n in ("groundtruth.txt", "pose.txt")) if os.path.isfile(p)), None)
        if pose_list is None:
            raise FileNotFoundError(f"{folder}: neither groundtruth.txt nor pose.txt")
        images, depths, poses = (_read_table(p) for p in (os.path.join(folder, "rgb.txt"), os.path.join(folder, "depth.txt"), pose_list))
        t_image = np.array([float(r[0]) for r in images])
        t_depth = np.array([float(r[0]) for r in depths])
        t_pose = np.array([float(r[0]) for r in poses])
        assoc = []
        for i, t in enumerate(t_image):
            j, k = int(np.argmin(np.abs(t_depth - t))), int(np.argmin(np.abs(t_pose - t)))
            if abs(t_depth[j] - t) < MAX_DT and abs(t_pose[k] - t) < MAX_DT:
                assoc.append((i, j, k))
        kept = assoc[:1]
        for a in assoc[1:]:
            if t_image[a[0]] - t_image[kept[-1][0]] > 1.0 / FRAME_RATE:
                kept.append(a)
        self.color_paths = [os.path.join(folder, images[i][1]) for i, _, _ in kept]
        self.depth_paths = [os.path.join(folder, depths[j][1]) for _, j, _ in kept]
        self.timestamps = [float(t_image[i]) for i, _, _ in kept]
        self.poses = []
        for _, _, k in kept:
            v = [float(x) for x in poses[k][1:8]]
            self.poses.append(np.linalg.inv(quaternion_pose(v[0:3], v[3:7])))
        self.n_img = len(self.color_paths)


class ReplicaParser:
    """``results/frame*.jpg`` + ``results/depth*.png`` (sorted, paired by position) and ``traj.txt`` with one row-major
    camera-to-world matrix per line; ``poses`` are their inverses."""

    def __init__(self, folder: str):
        self.input_folder = folder
        self.color_paths = sorted(glob.glob(os.path.join(folder, "results", "frame*.jpg")))
        self.depth_paths = sorted(glob.glob(os.path.join(folder, "results", "depth*.png")))
        self.n_img = len(self.color_paths)
        rows = _read_table(os.path.join(folder, "traj.txt"))
        if len(rows) < self.n_img:
            raise ValueError(f"{folder}/traj.txt holds {len(rows)} poses for {self.n_img} frames")
        self.poses = [np.linalg.inv(np.array([float(x) for x in rows[i]], dtype=np.float64).reshape(4, 4)) for i in range(self.n_img)]


# ---- dataset -----------------------------------------------------------------------------------------------------------------
class MonocularDataset:
    """The reference's ``MonocularDataset`` over a parser: ``dataset[i]`` decodes frame ``i`` with PIL and hands it to
    ``FrameIngest.prepare``.  Returns the reference's dict (``rgb`` float32 [3,H,W], ``depth`` float32 [H,W] or None, ``mask``
    bool, ``segmentation`` long or None, ``pose`` float64 [4,4] world-to-camera, all on ``device``) plus ``grad_mask``."""

    def __init__(self, parser, config: dict, device="cuda:0", preload: bool = False):
        cal = config["Dataset"]["Calibration"]
        self.calibration = dict(cal)
        self.device = device
        self.fx, self.fy, self.cx, self.cy = (float(cal[k]) for k in ("fx", "fy", "cx", "cy"))
        self.width, self.height = int(cal["width"]), int(cal["height"])
        self.K = np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])
        self.use_depth = bool(cal.get("use_depth", False))
        self.distorted = bool(cal["distorted"])
        self.depth_scale = cal.get("depth_scale")
        self.color_paths, self.depth_paths, self.poses = parser.color_paths, parser.depth_paths, parser.poses
        self.num_imgs = len(self.color_paths)
        self.has_depth = len(self.depth_paths) > 0
        if self.has_depth and self.use_depth and not self.depth_scale:
            raise ValueError("Calibration.depth_scale is needed to use the depth files")
        masked = (config["Dataset"].get("Objects") or {}).get("masked", ())
        self.ingest = FrameIngest(self.width, self.height, self.calibration, device, masked_ids=masked)
        self.preload = False
        self.color_imgs, self.depth_imgs = [], []
        if preload:
            self.load_data()

    def __len__(self):
        return self.num_imgs

    @property
    def with_depth(self) -> bool:
        return self.has_depth and self.use_depth

    def _decode(self, idx: int):
        from PIL import Image
        color = np.array(Image.open(self.color_paths[idx]))
        if color.ndim != 3 or color.shape[2] < 3:
            raise ValueError(f"{self.color_paths[idx]}: not a colour image")
        color = color[..., :3]                               # (the alpha channel is dropped)
        depth = np.array(Image.open(self.depth_paths[idx])) if self.with_depth and not getattr(self, "skip_depth", False) else None
        for a, p in ((color, self.color_paths[idx]), (depth, self.depth_paths[idx] if depth is not None else None)):
            if a is not None and a.shape[:2] != (self.height, self.width):
                raise ValueError(f"{p}: {a.shape[1]} x {a.shape[0]} pixels, the calibration says {self.width} x {self.height}")
        return color, depth

    def load_data(self):
        """Decode every frame up front (``load_data``, dataset.py:376-394); the device work stays per ``__getitem__``."""
        decoded = [self._decode(i) for i in range(self.num_imgs)]
        self.color_imgs, self.depth_imgs = [c for c, _ in decoded], [d for _, d in decoded]
        self.preload = True

    def __getitem__(self, idx: int) -> Dict[str, Optional[torch.Tensor]]:
        if not 0 <= idx < self.num_imgs:
            raise IndexError(idx)
        color, depth = (self.color_imgs[idx], self.depth_imgs[idx]) if self.preload else self._decode(idx)
        data = self.ingest.prepare(color, depth)
        data["pose"] = torch.from_numpy(np.asarray(self.poses[idx], dtype=np.float64)).to(self.device)
        return data


PARSERS = {"tum": TUMParser, "replica": ReplicaParser}


def load_dataset(config, device="cuda:0", preload: bool = False) -> MonocularDataset:
    """``config``: a path to a YAML or a dict with ``Dataset: {type, dataset_path, Calibration: {fx fy cx cy k1 k2 p1 p2 k3
    distorted width height depth_scale use_depth}}`` -- the reference's keys."""
    config = load_config(config)
    kind = config["Dataset"].get("type")
    if kind not in PARSERS:
        raise ValueError("Unknown dataset type")
    return MonocularDataset(PARSERS[kind](config["Dataset"]["dataset_path"]), config, device=device, preload=preload)


def config_is_monocular(config) -> bool:
    """``Dataset.sensor_type == "monocular"`` (the reference's configs/mono/* and configs/live/realsense.yaml)."""
    return (load_config(config).get("Dataset") or {}).get("sensor_type") == "monocular"


def dataset_frames(dataset: MonocularDataset, n_frames: int, device="cuda:0", start: int = 0, stride: int = 1,
                   monocular: bool = False, config=None, rgb_boundary_threshold: Optional[float] = None):
    """``(frames, intr)`` as ``sequences.make_room_sequence`` returns them: ``frames.Viewpoint`` objects over the frames ``start,
    start + stride, ...`` of the dataset, the ground-truth ``R`` / ``T`` from the world-to-camera pose and the ingest's ``mask``
    / ``grad_mask`` in place of recomputed ones.  ``monocular=True``: frames without depth (``Viewpoint(sensor="monocular")``, one
    shared all-zero depth image) from any dataset; depth files are not decoded.  ``config`` (a path or dict), where at hand:
    ``Dataset.sensor_type: monocular`` switches the mode on as well and ``Training.rgb_boundary_threshold`` (default 0.01) is the
    threshold of the frames' ``valid_rgb`` mask, unless the argument of that name gives one."""
    cfg = load_config(config) if config is not None else {}
    monocular = bool(monocular) or (config is not None and config_is_monocular(cfg))
    if rgb_boundary_threshold is None:
        rgb_boundary_threshold = float((cfg.get("Training") or {}).get("rgb_boundary_threshold", 0.01))
    if not monocular and not dataset.with_depth:
        raise ValueError("dataset_frames needs depth (depth files and Calibration.use_depth): the harness is RGB-D")
    idx = list(range(int(start), len(dataset), int(stride)))[:int(n_frames)]
    if len(idx) < int(n_frames):
        raise ValueError(f"the dataset holds {len(idx)} frames from {start} in steps of {stride}, {n_frames} were asked for")
    intr = Intrinsics(dict(fx=dataset.fx, fy=dataset.fy, cx=dataset.cx, cy=dataset.cy, W=dataset.width, H=dataset.height), device)
    frames = []
    zero = torch.zeros(dataset.height, dataset.width, dtype=torch.float32, device=device) if monocular else None
    was = getattr(dataset, "skip_depth", False)
    dataset.skip_depth = bool(monocular)                 # (the decode leaves the depth files alone)
    try:
        for n, i in enumerate(idx):
            d = dataset[i]
            pose = d["pose"].to(torch.float32)
            kw = dict(sensor="monocular", rgb_boundary_threshold=rgb_boundary_threshold) if monocular else {}
            frames.append(Viewpoint(n, d["rgb"], zero if monocular else d["depth"], device, gt_R=pose[:3, :3].contiguous(),
                                    gt_T=pose[:3, 3].contiguous(), mask=d["mask"], grad_mask=d["grad_mask"], **kw))
    finally:
        dataset.skip_depth = was
    return frames, intr
