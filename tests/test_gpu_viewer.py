"""The headless viewer on the device (pytest -m gpu): the ellipsoid walk against a float64 pick (tests/viewer_mirror.py), compose
bit for bit against numpy restatements of the reference's lines, the line overlay bit for bit against the integer mirror, and
``HeadlessViewer`` / ``run_slam(viewer_dir=...)`` end to end.  88 x 56 pixels (neither a multiple of 16) unless stated otherwise.

Tolerances of the walk: ``hit`` equal and colour within 1e-5 (float32 power and v_exp_f32 against float64: ~1e-6 on values <= 1)
on every pixel the mirror does not set aside; it sets aside a pixel whose decision hangs on rounding (a candidate's alpha within
1e-4 of the threshold, its power within 1e-6 of 0, the two front candidates' depths within 1e-5 relative), at most 2 % of them."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import viewer_mirror as vm
from monogs_amd.synthetic import make_scene, scene_settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = dict(fx=73.6, fy=74.1, cx=44.0, cy=27.6, W=88, H=56)
W, H = K["W"], K["H"]
THR = 0.4


def _from_camera_points(pc, sigma_px, opac, seed):
    """A scene of isotropic Gaussians at the camera-frame points ``pc`` whose projected sigma is ``sigma_px`` pixels."""
    P = pc.shape[0]
    sc = make_scene(P, K, seed=seed, near_fraction=0.0)
    return sc._replace(means3D=((pc - sc.t[None, :]) @ sc.R).contiguous(), scales=(sigma_px * pc[:, 2] / K["fx"])[:, None].contiguous(),
                       opacities=opac[:, None].contiguous())


def _scenes():
    g = torch.Generator().manual_seed(7)
    U = lambda n, a, b: a + (b - a) * torch.rand(n, generator=g)  # noqa: E731
    out = {"random400": make_scene(400, K, seed=5, anisotropic=True, near_fraction=0.02)}
    # one tile (2, 1) with a list longer than 64: 150 splats over pixels [34, 46] x [18, 30]
    n = 150
    z = U(n, 1.0, 4.0)
    pc = torch.stack([(U(n, 34.0, 46.0) + 0.5 - K["cx"]) / K["fx"] * z, (U(n, 18.0, 30.0) + 0.5 - K["cy"]) / K["fy"] * z, z], 1)
    out["long_list"] = _from_camera_points(pc, U(n, 1.5, 3.0), U(n, 0.05, 0.95), seed=11)
    # 24 co-located splats of opacity 0.39 in front of one of opacity 0.9, on the optical axis: the forward saturates before it
    # reaches the opaque one, and nothing else is in the image (empty tiles)
    z = torch.cat([2.0 + 0.01 * torch.arange(24), torch.tensor([3.0])])
    pc = torch.stack([torch.zeros(25), torch.zeros(25), z], 1)
    out["saturated"] = _from_camera_points(pc, torch.full((25,), 4.0), torch.cat([torch.full((24,), 0.39), torch.tensor([0.9])]), seed=13)
    return out


def _args(sc):
    d = lambda t: t.to(DEV)  # noqa: E731
    return dict(means3D=d(sc.means3D), opacities=d(sc.opacities), scales=d(sc.scales), rotations=d(sc.rotations))


@pytest.fixture(scope="module")
def cases(native_lib):
    """Per scene, computed once: the forward's tables, the mirror's pick, and the walk after an exact and a capacity-mode forward."""
    from monogs_amd import rasterizer as R
    from monogs_amd import viewer as V
    from monogs_amd.debug import forward_tables
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    out = {}
    R.check_overflow()
    for name, sc in _scenes().items():
        st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)
        a = _args(sc)
        tab = forward_tables(st, a["means3D"], a["opacities"], colors_precomp=sc.colors.to(DEV), scales=a["scales"],
                             rotations=a["rotations"])
        hit, color, aside = vm.ellipsoid_pick(tab["rec"].cpu().numpy(), (tab["radii"] > 0).cpu().numpy(), W, H, THR)
        got = {}
        P = sc.means3D.shape[0]
        try:
            for mode in ("exact", "capacity"):
                R.set_sync_free(mode == "capacity")
                col = sc.colors.to(DEV).requires_grad_(True)
                img = GaussianRasterizer(st)(means2D=torch.zeros(P, 3, device=DEV), colors_precomp=col, **a)[0]
                o, h = V.ellipsoids(img, THR)
                got[mode] = (o.cpu().numpy(), h.cpu().numpy())
            assert not R.check_overflow()
        finally:
            R.set_sync_free(False)
            R.forget_capacity(P, W, H)
        out[name] = dict(tab={k: (v.cpu() if torch.is_tensor(v) else v) for k, v in tab.items()}, hit=hit, color=color, aside=aside, got=got)
    return out


@pytest.mark.parametrize("name", ["random400", "long_list", "saturated"])
def test_the_mirror_sets_few_pixels_aside(cases, name):
    c = cases[name]
    frac = float(c["aside"].mean())
    print(f"{name}: {int(c['aside'].sum())} of {W * H} pixels set aside ({100 * frac:.2f} %), {int((c['hit'] >= 0).sum())} hits")
    assert frac <= 0.02
    assert (c["hit"] >= 0).any() and (c["hit"] < 0).any()


@pytest.mark.parametrize("mode", ["exact", "capacity"])
@pytest.mark.parametrize("name", ["random400", "long_list", "saturated"])
def test_ellipsoid_walk_matches_the_mirror(cases, name, mode):
    c = cases[name]
    out, hit = c["got"][mode]
    ok = ~c["aside"]
    err = np.abs(out - c["color"])[:, ok].max()
    wrong = int((hit != c["hit"])[ok].sum())
    print(f"{name} / {mode}: {wrong} wrong hits, colour error {err:.2e} on {int(ok.sum())} pixels")
    assert wrong == 0
    assert err <= 1e-5
    assert (out[:, hit < 0] == 0).all()                       # no hit: black
    # some pixel's hit is not the first entry of its tile's list: the walk walks
    rg, pl = c["tab"]["ranges"].numpy(), c["tab"]["point_list"].numpy()
    ys, xs = np.mgrid[0:H, 0:W]
    tile = (ys // 16) * ((W + 15) // 16) + xs // 16
    first = np.where(rg[tile, 1] > rg[tile, 0], pl[np.minimum(rg[tile, 0], max(len(pl) - 1, 0))], -1)
    assert ((hit >= 0) & (hit != first)).any()


def test_a_list_longer_than_one_step_is_walked(cases):
    c = cases["long_list"]
    rg = c["tab"]["ranges"].numpy()
    n = rg[:, 1] - rg[:, 0]
    assert n.max() > 64
    # a hit that sits beyond the first 64 entries of its tile's list
    pl, hit = c["tab"]["point_list"].numpy(), c["got"]["exact"][1]
    t = int(n.argmax())
    later = set(pl[rg[t, 0] + 64: rg[t, 1]].tolist()) - set(pl[rg[t, 0]: rg[t, 0] + 64].tolist())
    ty, tx = divmod(t, (W + 15) // 16)
    block = hit[ty * 16: ty * 16 + 16, tx * 16: tx * 16 + 16]
    assert np.isin(block, list(later)).any()


def test_the_hit_lies_beyond_the_forwards_stop_and_empty_tiles_stay_black(cases):
    c = cases["saturated"]
    tab = c["tab"]
    rg, pl, n_contrib = tab["ranges"].numpy(), tab["point_list"].numpy(), tab["n_contrib"].numpy()
    assert (rg[:, 1] == rg[:, 0]).any()                       # empty tiles
    py, px = 27, 44                                           # beside the projected centre (43.5, 27.1)
    for mode in ("exact", "capacity"):
        out, hit = c["got"][mode]
        assert hit[py, px] == 24                              # the opaque splat behind the 24 faint ones
        t = (py // 16) * ((W + 15) // 16) + px // 16
        pos = pl[rg[t, 0]: rg[t, 1]].tolist().index(24) + 1   # its 1-based list position
        assert pos == 25 and n_contrib[py, px] < pos, (pos, n_contrib[py, px])
        empty = np.repeat(np.repeat((rg[:, 1] == rg[:, 0]).reshape((H + 15) // 16, (W + 15) // 16), 16, 0), 16, 1)[:H, :W]
        assert (hit[empty] == -1).all() and (out[:, empty] == 0).all()


def test_no_gaussians_give_a_black_image_without_hits(native_lib):
    from monogs_amd.rasterizer import GaussianRasterizationSettings, _camera, _stream
    sc = make_scene(4, K, seed=1)
    keep = []
    cam = _camera(scene_settings(sc, GaussianRasterizationSettings, device=DEV), 0, keep, 3)
    out = torch.full((3, H, W), 7.0, device=DEV)
    hit = torch.full((H, W), 7, dtype=torch.int32, device=DEV)
    assert native_lib.mgs_viewer_ellipsoids(C.byref(cam), 0, 0, None, None, None, THR, out.data_ptr(), hit.data_ptr(), _stream()) == 0
    assert float(out.abs().max()) == 0.0 and bool((hit == -1).all())
    out.fill_(7.0)
    assert native_lib.mgs_viewer_ellipsoids(C.byref(cam), 0, 0, None, None, None, THR, out.data_ptr(), None, _stream()) == 0
    assert float(out.abs().max()) == 0.0


# ---- compose -------------------------------------------------------------------------------------------------------------------
def _scratch():
    from monogs_amd import _lib
    n = _lib.load().mgs_viewer_scratch_bytes(W, H)
    buf = torch.zeros(n + 256, dtype=torch.uint8, device=DEV)
    off = (-buf.data_ptr()) % 256
    return buf[off:off + n]


def _owner(scratch):
    return scratch[256:256 + W * H * 4].view(torch.int32).reshape(H, W)


@pytest.fixture(scope="module")
def images():
    g = np.random.default_rng(3)
    rgb = (g.random((3, H, W), dtype=np.float32) * 1.6 - 0.3).astype(np.float32)          # below 0 and above 1 too
    rgb[:, 0, :8] = np.array([0.0, 1.0, 0.5, 1.0 / 255, 254.5 / 255, 0.999999, -0.0, 2.0], dtype=np.float32)
    depth = (g.random((H, W), dtype=np.float32) * 5.0).astype(np.float32)
    depth[3, :5] = 0.0
    time = g.random((H, W), dtype=np.float32)
    time[0, :6] = np.array([np.nan, 1.5, 1.0, 0.0, -0.2, 255.5 / 256], dtype=np.float32)
    return dict(rgb=rgb, segmentation=rgb, elipsoids=rgb, depth=depth, time=time, depth0=np.zeros((H, W), np.float32))


@pytest.mark.parametrize("case", ["rgb", "segmentation", "elipsoids", "depth", "time", "depth0"])
def test_compose_is_bit_exact(native_lib, images, case):
    from monogs_amd import viewer as V
    mode = "depth" if case == "depth0" else case
    lut = V.jet_lut()
    got = V.compose(mode, torch.from_numpy(images[case]).to(DEV), torch.from_numpy(lut).to(DEV), None, _scratch()).cpu().numpy()
    want = vm.compose(mode, images[case], lut)
    assert got.shape == (H, W, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), int((got != want).sum())
    if case == "time":
        assert tuple(got[0, 0]) == (0, 0, 0) and tuple(got[0, 1]) == tuple(lut[255]) and tuple(got[0, 4]) == tuple(lut[0])
    if case == "depth0":
        assert (got == lut[0]).all()                             # left unnormalised: every pixel the table's first entry


# ---- lines -----------------------------------------------------------------------------------------------------------------------
SEGMENTS = np.array([
    [5 * 16, 10 * 16, 70 * 16, 10 * 16],            # horizontal
    [20 * 16, 2 * 16, 20 * 16, 50 * 16],            # vertical, crosses the first
    [10 * 16, 5 * 16, 40 * 16, 35 * 16],            # 45 degrees
    [40 * 16 + 3, 50 * 16 + 9, 2 * 16 - 5, 3 * 16 + 1],   # general, reversed, sub-pixel ends
    [60 * 16, 30 * 16, 200 * 16, 90 * 16],          # leaves the image
    [-300 * 16, 20 * 16 + 8, 500 * 16, 20 * 16 + 8],      # both ends outside, minor coordinate on a half: rounds up
    [50 * 16 + 2, 40 * 16 + 3, 50 * 16 + 6, 40 * 16 + 5],  # within one pixel
    [5 * 16, 10 * 16, 30 * 16, 10 * 16],            # over the first: the higher index wins
    [-50 * 16, -50 * 16, -20 * 16, -10 * 16],       # wholly outside
    [87 * 16, 0, 87 * 16, 55 * 16],                 # the last column
], dtype=np.int32)


def test_lines_are_bit_exact_and_the_highest_index_wins(native_lib, images):
    from monogs_amd import viewer as V
    scratch = _scratch()
    _owner(scratch).fill_(99)                                    # the call clears what an earlier frame left
    V.rasterize_lines(torch.from_numpy(SEGMENTS).to(DEV), scratch, W, H)
    want = vm.lines_owner(SEGMENTS, W, H)
    got = _owner(scratch).cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    assert got[10, 20] == 8 and got[10, 40] == 1 and got[21, 0] == 6 and got[40, 50] == 7 and (got[:, 87] == 10).all()
    # compose resolves it over every mode's image
    seg_rgb = np.random.default_rng(1).integers(0, 256, (len(SEGMENTS), 3), dtype=np.uint8)
    lut = V.jet_lut()
    for mode in ("rgb", "depth", "time", "elipsoids"):
        img = V.compose(mode, torch.from_numpy(images[mode]).to(DEV), torch.from_numpy(lut).to(DEV), torch.from_numpy(seg_rgb).to(DEV),
                        scratch).cpu().numpy()
        assert np.array_equal(img, vm.compose(mode, images[mode], lut, want, seg_rgb)), mode
    # zero segments: the owner image is cleared and nothing is drawn
    V.rasterize_lines(torch.zeros(0, 4, dtype=torch.int32, device=DEV), scratch, W, H)
    assert int(_owner(scratch).abs().max()) == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
ROOM = dict(n_frames=12, intrinsics=dict(fx=535.4 / 4, fy=539.2 / 4, cx=320.1 / 4, cy=247.6 / 4, W=160, H=120),
            tracking_itr_num=100, mapping_itr_num=60, init_itr_num=600, window_size=4, kf_interval=2, scene="room")
ALL_MODES = ("rgb", "segmentation", "depth", "time", "elipsoids")


def _key_shape(d, prefix=""):
    out = {}
    for k, v in d.items():
        out[prefix + k] = v is None
        if isinstance(v, dict) and all(isinstance(x, str) for x in v):
            out.update(_key_shape(v, prefix + k + "."))
    return out


@pytest.fixture(scope="module")
def room_run(native_lib, tmp_path_factory):
    from monogs_amd.slam_harness import run_slam
    d = tmp_path_factory.mktemp("viewer")
    return d, run_slam(nr_objects=18, viewer_dir=str(d), viewer_modes=ALL_MODES, viewer_every=3, **ROOM)


def test_run_slam_writes_the_frames_and_reports_them(room_run):
    from PIL import Image
    d, r = room_run
    tags = [f"kf{k:04d}" for k in range(3, r["keyframes"] + 1, 3)] + ["final"]
    want = [os.path.join(str(d), f"{t}_{m}.png") for t in tags for m in ALL_MODES]
    assert r["viewer"] == dict(dir=str(d), modes=list(ALL_MODES), every=3, files=want)
    for path in want:
        img = np.asarray(Image.open(path))
        assert img.shape == (120, 160, 3) and img.dtype == np.uint8 and img.max() > 0, path
    final = np.asarray(Image.open(os.path.join(str(d), "final_rgb.png")))
    assert (final == (0, 255, 0)).all(-1).any() and (final == (255, 255, 0)).all(-1).any()       # the current camera, the keyframes
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_slam_contract.json")) as f:
        rec = json.load(f)["objects"]["keys"]
    now = _key_shape(r)
    assert {k: v for k, v in now.items() if k != "viewer" and not k.startswith("viewer.")} == rec


def test_run_slam_without_a_viewer_dir_keeps_its_keys(native_lib):
    from monogs_amd.slam_harness import run_slam
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_slam_contract.json")) as f:
        rec = json.load(f)["eager"]["keys"]
    assert _key_shape(run_slam(**ROOM)) == rec


def test_frames_replay_from_a_graph_bit_for_bit(room_run):
    from monogs_amd import rasterizer as R
    from monogs_amd import viewer as V
    _, r = room_run
    gmap, intr, frames = r["map"], r["intr"], r["frame_list"]
    snap = V.Snapshot.from_map(gmap, frames[::2], current=frames[-1], gt=frames[-1])
    assert snap.obj_idx is not None and snap.obj_idx.shape[0] == len(gmap)
    hv = V.HeadlessViewer(intr, torch.zeros(3, device=DEV))
    cam = V.view_behind(frames[-1], intr, size=0.5)
    R.check_overflow()
    try:
        for mode in ALL_MODES:
            want_hit = mode == "elipsoids"
            eager = hv.frame(snap, cam, mode=mode, want_hit=want_hit)
            eager = [t.clone() for t in (eager if want_hit else (eager,))]
            assert eager[0].shape == (120, 160, 3) and eager[0].dtype == torch.uint8 and int(eager[0].max()) > 0
            handle, graph = R.graph_flags(), torch.cuda.CUDAGraph()
            with handle, torch.cuda.graph(graph):
                out = hv.frame(snap, cam, mode=mode, want_hit=want_hit)
            out = out if want_hit else (out,)
            for _ in range(2):
                for t in out:
                    t.zero_()
                graph.replay()
                torch.cuda.synchronize()
                for a, b in zip(out, eager):
                    assert torch.equal(a, b), mode
            assert not R.check_overflow()
            handle.release()
            del graph
            if want_hit:
                assert int((eager[1] >= 0).sum()) > 0 and int(eager[1].max()) < len(gmap)
        # the overlay is part of every frame, and can be left out
        plain = hv.frame(snap, cam, mode="rgb", cameras=False, trajectory=False)
        with_lines = hv.frame(snap, cam, mode="rgb")
        assert not torch.equal(plain, with_lines) and bool((with_lines == torch.tensor([0, 255, 0], device=DEV, dtype=torch.uint8)).all(-1).any())
        # a free orbit renders too
        c0 = V.orbit(snap.means.mean(0).cpu().numpy(), 1.5, 4)[1]
        assert int(hv.frame(snap, c0, mode="depth", scale_modifier=0.5).max()) > 0
    finally:
        R.clear_graph_flags()
        R.forget_capacity(len(gmap), 160, 120)
