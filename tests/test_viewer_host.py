"""Host side of the headless viewer (monogs_amd/viewer.py, the v20 entry points): ABI agreement, argument errors that come back
before any launch, the jet table against the matplotlib recording, the frustum formula, clipping and quantisation against
tests/viewer_mirror.py, the Python errors.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import viewer_mirror as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mgs_viewer_scratch_bytes", "mgs_viewer_ellipsoids", "mgs_viewer_lines", "mgs_viewer_compose")
K = dict(fx=73.6, fy=74.1, cx=44.0, cy=27.6, W=88, H=56)


class _Intr:
    def __init__(self, k):
        self.fx, self.fy, self.cx, self.cy, self.width, self.height = k["fx"], k["fy"], k["cx"], k["cy"], k["W"], k["H"]


def test_header_signatures_and_library_agree(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 20
    assert native_lib.mgs_abi_version() == _lib.ABI_VERSION
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    for name, value in (("RGB", 0), ("DEPTH", 1), ("TIME", 2), ("ELLIPSOIDS", 3)):
        assert re.search(r"#define MGS_VIEWER_%s %d\b" % (name, value), text)


def _cam(W=16, H=16):
    from monogs_amd import _lib
    cam = _lib.MgsCamera()
    cam.image_height, cam.image_width = H, W
    for f in ("bg", "viewmatrix", "projmatrix", "projmatrix_raw", "campos"):
        setattr(cam, f, 0x1000)                      # non-NULL and never dereferenced: every call below is refused first
    return cam


def test_entry_points_refuse_bad_arguments_before_any_launch(native_lib):
    lib, p = native_lib, 0x1000                      # (a pointer that is never dereferenced)
    assert lib.mgs_viewer_scratch_bytes(0, 16) == 0 and lib.mgs_viewer_scratch_bytes(16, -1) == 0
    assert lib.mgs_viewer_scratch_bytes(88, 56) >= 256 + 88 * 56 * 4
    cam = _cam()
    ell = lib.mgs_viewer_ellipsoids
    assert ell(None, 1, 1, p, p, p, 0.4, p, None, None) == 1                       # no camera
    assert ell(C.byref(_cam(0, 16)), 1, 1, p, p, p, 0.4, p, None, None) == 1         # non-positive size
    assert ell(C.byref(cam), -1, 1, p, p, p, 0.4, p, None, None) == 1
    assert ell(C.byref(cam), 1, 1, p, p, p, 0.4, None, None, None) == 1            # out
    assert ell(C.byref(cam), 1, 1, None, p, p, 0.4, p, None, None) == 1            # geometry
    assert ell(C.byref(cam), 1, 1, p, p, None, 0.4, p, None, None) == 1            # image
    assert ell(C.byref(cam), 1, 1, p, None, p, 0.4, p, None, None) == 1            # binning with instances
    for thr in (0.0, 1.0, float("nan")):
        assert ell(C.byref(cam), 1, 1, p, p, p, thr, p, None, None) == 1
    assert ell(C.byref(cam), 1 << 26, 1, p, p, p, 0.4, p, None, None) == 1 and b"MGS_MAX_GAUSSIANS" in lib.mgs_last_error()
    lines = lib.mgs_viewer_lines
    assert lines(0, 16, p, 1, 0x1000, None) == 1 and lines(16, 0, p, 1, 0x1000, None) == 1
    assert lines(16, 16, None, 1, 0x1000, None) == 1 and lines(16, 16, p, -1, 0x1000, None) == 1
    assert lines(16, 16, p, 1, None, None) == 1 and lines(16, 16, p, 1, 0x1004, None) == 1      # scratch: NULL, misaligned
    comp = lib.mgs_viewer_compose
    for mode in (-1, 4, 99):
        assert comp(mode, 16, 16, p, p, None, 0, 0x1000, p, None) == 1 and b"mode" in lib.mgs_last_error()
    assert comp(0, 0, 16, p, p, None, 0, 0x1000, p, None) == 1 and comp(0, 16, -3, p, p, None, 0, 0x1000, p, None) == 1
    assert comp(0, 16, 16, None, p, None, 0, 0x1000, p, None) == 1 and comp(0, 16, 16, p, p, None, 0, 0x1000, None, None) == 1
    assert comp(1, 16, 16, p, None, None, 0, 0x1000, p, None) == 1 and comp(2, 16, 16, p, None, None, 0, 0x1000, p, None) == 1
    assert comp(1, 16, 16, p, p, None, 0, None, p, None) == 1                      # depth needs the scratch
    assert comp(0, 16, 16, p, p, None, 2, 0x1000, p, None) == 1                    # segments without colours
    assert comp(0, 16, 16, p, p, p, 2, None, p, None) == 1 and comp(0, 16, 16, p, p, p, -1, 0x1000, p, None) == 1


def test_jet_table_equals_the_matplotlib_recording():
    from monogs_amd.viewer import jet_lut
    want = np.load(os.path.join(ROOT, "tests", "golden", "jet_lut.npy"))
    got = jet_lut()
    assert want.shape == (256, 3) and want.dtype == np.uint8
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert tuple(got[0]) == (0, 0, 127) and tuple(got[255]) == (127, 0, 0)


def test_frustum_points_and_lines():
    from monogs_amd.viewer import FreeCamera, frustum_points, frustum_segments, look_at, trajectory_segments
    cam = look_at((0.3, -0.2, -1.0), (0.1, 0.0, 2.0), (0.0, -1.0, 0.1))
    assert np.allclose(cam.R @ cam.R.T, np.eye(3), atol=1e-12) and np.linalg.det(cam.R) > 0
    assert np.allclose(cam.R @ np.array([0.3, -0.2, -1.0]) + cam.T, 0.0, atol=1e-12)          # the eye is the camera centre
    tgt = cam.R @ np.array([0.1, 0.0, 2.0]) + cam.T
    assert abs(tgt[0]) < 1e-12 and abs(tgt[1]) < 1e-12 and tgt[2] > 0                         # the target on the optical axis
    for size in (1.0, 0.35):
        got = frustum_points(cam.c2w, _Intr(K), size)
        assert np.array_equal(got, vm.frustum_points(cam.c2w, K, size))
        # in the camera frame: the apex at the centre, the corners at depth max(fx, fy) * 1e-3 * size
        back = (got - cam.c2w[:3, 3]) @ cam.c2w[:3, :3]
        assert np.allclose(back[0], 0.0, atol=1e-12) and np.allclose(back[1:, 2], max(K["fx"], K["fy"]) * 1e-3 * size)
        segs = frustum_segments(cam.c2w, _Intr(K), size)
        assert segs.shape == (8, 2, 3)
        pairs = [[0, 1], [0, 2], [0, 3], [0, 4], [1, 2], [1, 3], [2, 4], [3, 4]]
        assert np.array_equal(segs, np.stack([got[p] for p in pairs]))
    t = trajectory_segments([[0, 0, 0], [1, 0, 0], [1, 2, 0]])
    assert t.shape == (2, 2, 3) and np.array_equal(t[1], [[1, 0, 0], [1, 2, 0]])
    assert trajectory_segments([[0, 0, 0]]).shape == (0, 2, 3)
    assert FreeCamera.of((cam.R, cam.T)).c2w.shape == (4, 4)


def test_clipping_and_quantisation_against_the_mirror():
    from monogs_amd.viewer import FreeCamera, project_segments
    cam = FreeCamera(np.eye(3), np.zeros(3))
    segs = np.array([
        [[0.0, 0.0, -1.0], [0.5, 0.2, 0.1]],            # wholly behind the near plane: dropped
        [[0.1, 0.05, -0.5], [-0.2, 0.1, 1.5]],          # crosses the near plane: clipped
        [[900.0, 0.1, 1.0], [1000.0, -0.2, 1.2]],       # far outside: dropped by the guard rectangle
        [[-0.3, 0.02, 1.0], [40.0, 0.3, 1.1]],          # leaves the guard rectangle: clipped to it
        [[0.01, 0.01, 2.0], [0.0102, 0.0101, 2.0]],     # sub-pixel: survives
    ])
    got = project_segments(segs, cam, _Intr(K))
    want = [vm.project_segment(p, q, cam.R, cam.T, K) for p, q in segs]
    assert want[0] is None and want[2] is None and all(w is not None for w in (want[1], want[3], want[4]))
    assert [int(r[4]) for r in got] == [1, 3, 4]
    for row in got:
        assert tuple(int(v) for v in row[:4]) == want[int(row[4])]
    # the clipped one ends ON the near plane, the guarded one ON the guard rectangle, the sub-pixel one inside one pixel
    p, q = segs[1]
    t = (0.2 - p[2]) / (q[2] - p[2])
    on = p + t * (q - p)
    assert abs(got[0][0] / 16.0 - (K["fx"] * on[0] / 0.2 + K["cx"] - 0.5)) <= 1.0 / 16
    assert got[1][2] == (K["W"] + 1024) * 16
    assert np.abs(got[2][:2] - got[2][2:4]).max() < 16 and len(vm.segment_pixels(*got[2][:4])) == 1
    assert project_segments(np.zeros((0, 2, 3)), cam, _Intr(K)).shape == (0, 5)


def test_line_rule_of_the_mirror():
    """The normative rule on cases small enough to check by hand."""
    assert vm.segment_pixels(0, 0, 48, 0) == [(0, 0), (1, 0), (2, 0), (3, 0)]                 # horizontal, ends on centres
    assert vm.segment_pixels(8, 0, 40, 0) == [(1, 0), (2, 0)]                                 # ends between centres: inside only
    assert vm.segment_pixels(16, 48, 16, 0) == [(1, 0), (1, 1), (1, 2), (1, 3)]               # vertical, reversed
    assert vm.segment_pixels(0, 0, 32, 32) == [(0, 0), (1, 1), (2, 2)]                        # 45 degrees: x is the major axis
    assert vm.segment_pixels(0, 0, 32, 8) == [(0, 0), (1, 0), (2, 1)]                         # minor 4/16 -> 0, 8/16 -> 1 (half up)
    assert vm.segment_pixels(-32, -8, 0, 0) == [(-2, 0), (-1, 0), (0, 0)]                     # -8/16 -> 0 (half up), -4/16 -> 0
    assert vm.segment_pixels(3, 5, 9, 7) == [(0, 0)] and vm.segment_pixels(24, 40, 24, 40) == [(2, 3)]
    own = vm.lines_owner([[0, 0, 48, 0], [16, 0, 16, 32], [-64, 16, 4000, 16]], 4, 3)
    assert own.tolist() == [[1, 2, 1, 1], [3, 3, 3, 3], [0, 2, 0, 0]]


def test_python_errors_are_raised_before_the_library_is_touched():
    from monogs_amd import viewer as V
    snap = V.Snapshot(*(torch.zeros(4, n) for n in (3, 4, 1, 1, 3)), None, (), None, None)
    hv = V.HeadlessViewer(_Intr(K), torch.zeros(3))
    cam = V.FreeCamera(np.eye(3), np.zeros(3))
    with pytest.raises(ValueError, match="unknown viewer mode"):
        hv.frame(snap, cam, mode="ellipsoids")                      # (the reference's spelling is the mode's name)
    with pytest.raises(ValueError, match="object layer"):
        hv.frame(snap, cam, mode="segmentation")
    with pytest.raises(RuntimeError, match="no CPU path"):
        hv.frame(snap, cam, mode="rgb")
    with pytest.raises(ValueError, match="want_hit"):
        hv.frame(snap, cam, mode="depth", want_hit=True)
    with pytest.raises(ValueError, match="unknown viewer mode"):
        V.compose("jet", torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.compose("rgb", torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.rasterize_lines(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(512, dtype=torch.uint8), 4, 4)
    with pytest.raises(ValueError, match="parallel"):
        V.look_at((0, 0, 0), (0, 0, 1), (0, 0, 2))
    assert len(V.orbit((0, 0, 2), 1.5, 5)) == 5


def test_the_viewer_module_stands_beside_the_harness():
    import ast
    with open(os.path.join(ROOT, "monogs_amd", "viewer.py")) as f:
        src = f.read()
    names = []
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            names += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            names += [node.module or ""] + [a.name for a in node.names]
    assert not [n for n in names if "slam_harness" in n.split(".")]
    assert "mgs_activate" not in src
