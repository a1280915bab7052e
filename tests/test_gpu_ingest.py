"""The frame ingest (csrc/ingest.hip, monogs_amd/frame_ingest.py, monogs_amd/dataset.py) on the GPU (pytest -m gpu).

Bars.  Colour, depth, remap and the segmentation mask are integer or correctly-rounded conversions: exact equality with the
mirror (tests/ingest_mirror.py).  The gradient intensity is held to 1e-6 absolute: fewer than ten float32 roundings of terms
bounded by 1 (the reference's own float32 result sits 7e-8 from a float64 evaluation).  The gradient mask must equal the
reference's / the mirror's at every pixel whose float64 intensity is more than 2e-6 away from 1.1 x the float64 median -- twice
the intensity bound -- and at most 8 pixels of an image may fall inside that band (the reference's own masks of the golden
images leave out 0, 4 and 1).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import ingest_mirror as im

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Dataset.Calibration of the reference's configs/rgbd/tum/fr1_desk.yaml
FR1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628,
           k3=1.163314, distorted=True, width=640, height=480, depth_scale=5000.0)
INTENSITY_TOL, BAND, MAX_IN_BAND = 1e-6, 2e-6, 8


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _prepare(rgb, maps=None, depth=None, scale=5000.0, seg=None, ids=(), fill=0):
    """``mgs_frame_prepare`` through the C ABI on freshly uploaded inputs; scratch and every output are pre-filled with the byte
    ``fill``.  Returns numpy arrays."""
    from monogs_amd import _lib
    from monogs_amd.frame_ingest import masked_id_words
    from monogs_amd.rasterizer import _stream
    lib = _lib.load()
    H, W = rgb.shape[:2]

    def full(shape, dt):
        n = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        return torch.full((n,), fill, dtype=torch.uint8, device=DEV).view(dt).view(shape)

    out = dict(rgb=full((3, H, W), torch.float32), mask=full((H, W), torch.uint8), grad_mask=full((H, W), torch.uint8),
               intensity=full((H, W), torch.float32), depth=full((H, W), torch.float32))
    scratch = torch.full((lib.mgs_grad_mask_scratch_bytes(W, H),), fill, dtype=torch.uint8, device=DEV)
    keep = [_dev(rgb), _dev(depth), _dev(seg)] + ([_dev(maps[0]), _dev(maps[1])] if maps is not None else [None, None])
    p = _lib.MgsFramePrepare()
    p.width, p.height = W, H
    p.rgb_u8 = keep[0].data_ptr()
    if depth is not None:
        p.depth_u16, p.depth_out, p.depth_scale = keep[1].data_ptr(), out["depth"].data_ptr(), scale
    if seg is not None:
        p.segmentation = keep[2].data_ptr()
    if maps is not None:
        p.map_x, p.map_y = keep[3].data_ptr(), keep[4].data_ptr()
    p.masked_ids = (C.c_uint32 * 8)(*masked_id_words(ids))
    p.rgb_out, p.mask_out, p.grad_mask_out = out["rgb"].data_ptr(), out["mask"].data_ptr(), out["grad_mask"].data_ptr()
    p.intensity_out = out["intensity"].data_ptr()
    p.edge_threshold, p.eps = 1.1, 0.01
    p.scratch = scratch.data_ptr()
    assert lib.mgs_frame_prepare(C.byref(p), _stream()) == 0, lib.mgs_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def _check_grad_mask(name, got_intensity, got_mask, ref_intensity64, ref_mask, check_mask=True):
    """The bars of the module docstring against a float64 intensity and the mask that goes with it."""
    err = np.abs(got_intensity.astype(np.float64) - ref_intensity64).max()
    thr = im.lower_median(ref_intensity64) * 1.1
    band = np.abs(ref_intensity64 - thr) <= BAND
    wrong = int(((got_mask != 0) != ref_mask)[~band].sum())
    print(f"{name}: intensity error {err:.3e}, {int(band.sum())} pixels in the band, {wrong} mismatches outside it")
    assert err <= INTENSITY_TOL, (name, err)
    if check_mask:
        assert band.sum() <= MAX_IN_BAND, (name, int(band.sum()))
        assert wrong == 0, (name, wrong)
        assert set(np.unique(got_mask)) <= {0, 1}


# ---- colour and depth --------------------------------------------------------------------------------------------------------
def test_colour_conversion_is_the_float64_division_rounded_once(native_lib):
    vals = np.stack([np.random.default_rng(c).permutation(256) for c in range(3)], axis=-1).astype(np.uint8)     # [256, 3]
    vec = vals.reshape(16, 16, 3)                                    # 16 x 16: the vector route
    sca = _noise(23, 37, 5)                                          # 37 x 23: the scalar route
    sca.reshape(-1, 3)[100:356] = vals
    for img in (vec, sca):
        got = _prepare(img)["rgb"]
        ref = np.float32(img.astype(np.float64) / 255.0).transpose(2, 0, 1)
        assert (_bits(got) == _bits(ref)).all()
        assert all(set(np.unique(img[..., c])) == set(range(256)) for c in range(3))


@pytest.mark.parametrize("scale", [5000.0, 6553.5])
def test_depth_conversion_over_all_16_bit_values(native_lib, scale):
    d = np.random.default_rng(3).permutation(65536).astype(np.uint16).reshape(256, 256)
    got = _prepare(_noise(256, 256, 4), depth=d, scale=scale)["depth"]
    assert (_bits(got) == _bits(np.float32(d.astype(np.float64) / scale))).all()


# ---- remap -------------------------------------------------------------------------------------------------------------------
def _special_map():
    """37 x 23 maps: a smooth warp, then the values that sit on the rules' edges written over some of its entries."""
    W, H = 37, 23
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    rng = np.random.default_rng(7)
    mx = (xx + rng.uniform(-1.5, 1.5, (H, W))).astype(np.float32)
    my = (yy + rng.uniform(-1.5, 1.5, (H, W))).astype(np.float32)
    special_x = [5.0, W - 1, W - 1 + 1 / 32, -1 / 64, -0.5, -1.0, -1.5, 1e9, -1e9, np.inf, -np.inf, np.nan, W - 1 + 31 / 32, float(W)]
    special_y = [7.0, H - 1, H - 1 + 1 / 32, -1 / 64, -0.5, -1.0, -1.5, 1e9, -1e9, np.inf, -np.inf, np.nan, H - 1 + 31 / 32, float(H)]
    for k, v in enumerate(special_x):
        mx[2, k] = v                     # against an ordinary y
        mx[4, k] = v
        my[4, k] = special_y[k]          # against the same kind of y
    for k, v in enumerate(special_y):
        my[6, k] = v                     # against an ordinary x
        mx[8 + k % 3, 20 + k] = special_x[(k + 5) % len(special_x)]
        my[8 + k % 3, 20 + k] = v        # mixed pairs
    return mx, my


def test_remap_is_bit_exact_against_the_integer_mirror(native_lib):
    from monogs_amd.frame_ingest import undistort_map
    s = 1.0 / 8.0
    fr1 = undistort_map(FR1["fx"] * s, FR1["fy"] * s, FR1["cx"] * s, FR1["cy"] * s, FR1["k1"], FR1["k2"], FR1["p1"], FR1["p2"], FR1["k3"], 80, 60)
    outside = (fr1[0] < 0) | (fr1[0] > 79) | (fr1[1] < 0) | (fr1[1] > 59)
    assert 0.05 < outside.mean() < 0.12 and fr1[0].min() < 0 and fr1[0].max() > 79 and fr1[1].min() < 0 and fr1[1].max() > 59
    tiny = (np.array([[-0.5, 1.25], [0.5, 0.96875]], np.float32), np.array([[0.0, -0.25], [1.0, 0.5]], np.float32))
    for name, img, maps in (("fr1_desk / 8", _noise(60, 80, 11), fr1), ("special", _noise(23, 37, 12), _special_map()),
                            ("2 x 2", _noise(2, 2, 13), tiny)):
        got = _prepare(img, maps=maps)["rgb"]
        ref = im.colour(im.remap_u8(img, *maps))
        assert (_bits(got) == _bits(ref)).all(), (name, int((_bits(got) != _bits(ref)).sum()))


def test_integer_remap_stays_within_one_grey_level_of_true_bilinear(native_lib):
    """1/2 for the final rounding plus 1/64 pixel of coordinate quantisation per axis times a slope of at most 2 grey levels per
    pixel: well inside 1 (the mirror measures 0.54 on this input)."""
    W, H = 37, 23
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([2 * xx + yy, xx + 2 * yy, 2 * xx], axis=-1).astype(np.uint8)              # no wrap: at most 2 * 36 + 22
    rng = np.random.default_rng(0)
    mx = (xx + rng.uniform(-3, 3, (H, W))).astype(np.float32)
    my = (yy + rng.uniform(-3, 3, (H, W))).astype(np.float32)
    got = _prepare(img, maps=(mx, my))["rgb"].transpose(1, 2, 0).astype(np.float64) * 255.0
    ref = im.bilinear_f64(img, mx, my)
    inside = ~np.isnan(ref)
    err = np.abs(got - ref)[inside].max()
    print(f"integer remap vs float64 bilinear: {err:.3f} grey levels over {inside.mean():.0%} of the pixels")
    assert inside.mean() > 0.5 and err <= 1.0


# ---- gradient mask -----------------------------------------------------------------------------------------------------------
def test_grad_mask_against_the_reference_outputs(native_lib):
    from monogs_amd.frame_ingest import grad_mask
    gold = np.load(os.path.join(ROOT, "tests", "golden", "grad_mask.npz"))
    for i in range(3):
        img = gold["images"][i]
        mask, intensity = grad_mask(torch.from_numpy(img).to(DEV), return_intensity=True)
        assert mask.dtype == torch.bool and mask.shape == (60, 80)
        ref64 = im.intensity(img)
        got = intensity.cpu().numpy()
        err = np.abs(got - gold[f"intensity_{i}"][0]).max()
        print(f"image {i}: {err:.3e} from the reference's float32 intensity")
        assert err <= INTENSITY_TOL
        _check_grad_mask(f"golden image {i}", got, mask.cpu().numpy(), ref64, gold[f"mask_{i}"][0])
        assert torch.equal(grad_mask(torch.from_numpy(img).to(DEV)), mask)


def _blocked(seed):
    """60 x 80 noise with a black block and black pixels on and next to all four borders: the 3 x 3 validity rule decides."""
    img = _noise(60, 80, seed)
    img[20:40, 30:60] = 0
    img[0, 10] = img[59, 70] = img[30, 0] = img[45, 79] = 0
    img[1, 20] = img[58, 5] = img[12, 1] = img[50, 78] = 0
    img[0, 0] = img[59, 79] = 0
    return img


@pytest.mark.parametrize("shape", ["37x23", "5x4", "60x80 blocked", "2x2"])
def test_grad_mask_other_shapes_against_the_float64_mirror(native_lib, shape):
    img = {"37x23": _noise(23, 37, 21), "5x4": _noise(4, 5, 22), "60x80 blocked": _blocked(23), "2x2": _noise(2, 2, 24)}[shape]
    out = _prepare(img)
    ref_rgb = im.colour(img)
    assert (_bits(out["rgb"]) == _bits(ref_rgb)).all()
    it, _, mask = im.grad_mask(ref_rgb)
    if shape == "60x80 blocked":
        assert (it[21:39, 31:59] == 0).all() and (it[19:41, 29:61] == 0).all() and it[18, 40] > 0      # one pixel around the block
        assert it[0, 9] == it[0, 11] == it[1, 10] == 0 and it[31, 1] == 0 and it[0, 1] == 0 and it[58, 78] == 0
    _check_grad_mask(shape, out["intensity"], out["grad_mask"], it, mask, check_mask=shape != "2x2")


# ---- segmentation, optional inputs, stale state --------------------------------------------------------------------------------
def test_segmentation_mask_and_optional_inputs(native_lib):
    img = _noise(23, 37, 31)
    seg = np.random.default_rng(32).integers(0, 256, size=(23, 37), dtype=np.uint8)
    seg.reshape(-1)[50:306] = np.arange(256, dtype=np.uint8)
    out = _prepare(img, seg=seg, ids=(0, 7, 255), fill=0xFF)
    assert (out["mask"].astype(bool) == im.mask(seg, (0, 7, 255))).all() and set(np.unique(out["mask"])) == {0, 1}
    assert (out["mask"] == 0).sum() >= 3
    # 16-byte route: 40 x 24
    img4, seg4 = _noise(24, 40, 33), np.random.default_rng(34).integers(0, 256, size=(24, 40), dtype=np.uint8)
    seg4.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    ids = (1, 31, 32, 63, 64, 100, 128, 191, 192, 254)
    assert (_prepare(img4, seg=seg4, ids=ids)["mask"].astype(bool) == im.mask(seg4, ids)).all()
    # no segmentation: all ones, whatever the set; no depth: depth_out is not written
    out = _prepare(img, ids=(0, 7, 255), fill=0xAB)
    assert (out["mask"] == 1).all()
    assert (out["depth"].view(np.uint8) == 0xAB).all()


@pytest.mark.parametrize("shape", [(24, 40), (23, 37)])
def test_results_do_not_depend_on_what_scratch_and_outputs_held(native_lib, shape):
    H, W = shape
    img, depth = _noise(H, W, 41), np.random.default_rng(42).integers(0, 65536, size=(H, W), dtype=np.uint16)
    seg = np.random.default_rng(43).integers(0, 4, size=(H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    maps = (xx + 0.3, yy - 0.7)
    a = _prepare(img, maps=maps, depth=depth, seg=seg, ids=(2,), fill=0x00)
    b = _prepare(img, maps=maps, depth=depth, seg=seg, ids=(2,), fill=0xFF)
    for k in a:
        assert (a[k].view(np.uint8) == b[k].view(np.uint8)).all(), k


# ---- capture -----------------------------------------------------------------------------------------------------------------
def _frame(seed, H=60, W=80):
    return _noise(H, W, seed), np.random.default_rng(seed + 100).integers(0, 65536, size=(H, W), dtype=np.uint16)


def _capture(fi, keep_graph=False):
    ins = fi.static_inputs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fi.prepare_device(ins["rgb"], ins["depth"])          # (the code objects are loaded before the capture)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph(keep_graph=True) if keep_graph else torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fi.prepare_device(ins["rgb"], ins["depth"])
    return g, ins, out


def test_captured_prepare_replays_on_new_contents(native_lib):
    from monogs_amd.frame_ingest import FrameIngest
    cal = dict(FR1, **{k: FR1[k] / 8 for k in ("fx", "fy", "cx", "cy")}, width=80, height=60)
    fi = FrameIngest(80, 60, cal, DEV)
    (rgb1, d1), (rgb2, d2) = _frame(51), _frame(52)
    eager = [fi.prepare(rgb, d) for rgb, d in ((rgb1, d1), (rgb2, d2))]
    eager = [{k: v.clone() for k, v in e.items() if v is not None} for e in eager]
    assert eager[0]["mask"].dtype == eager[0]["grad_mask"].dtype == torch.bool and eager[0]["rgb"].shape == (3, 60, 80)
    assert not torch.equal(eager[0]["rgb"], eager[1]["rgb"])
    g, ins, out = _capture(fi)
    for rgb, d, ref in ((rgb1, d1, eager[0]), (rgb2, d2, eager[1]), (rgb1, d1, eager[0])):
        ins["rgb"].copy_(torch.from_numpy(rgb)); ins["depth"].copy_(torch.from_numpy(d))
        g.replay()
        torch.cuda.synchronize()
        for k in ("rgb", "depth", "mask", "grad_mask"):
            assert torch.equal(out[k].view(torch.uint8), ref[k].view(torch.uint8)), k


def _hip_runtime():
    """The HIP runtime this process already runs on (never a second copy)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not mapped")


def test_prepare_is_at_most_nine_kernel_nodes(native_lib):
    from monogs_amd.frame_ingest import FrameIngest
    cal = dict(FR1, **{k: FR1[k] / 8 for k in ("fx", "fy", "cx", "cy")}, width=80, height=60)
    fi = FrameIngest(80, 60, cal, DEV)
    g, ins, out = _capture(fi, keep_graph=True)
    hip = _hip_runtime()
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(C.c_void_p(g.raw_cuda_graph()), None, C.byref(n)) == 0
    nodes = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(C.c_void_p(g.raw_cuda_graph()), nodes, C.byref(n)) == 0
    kinds = []
    for node in nodes:
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(t)) == 0
        kinds.append(t.value)
    print("graph nodes:", n.value, "types:", kinds)
    assert 1 <= n.value <= 9 and set(kinds) == {0}, kinds            # hipGraphNodeTypeKernel = 0: no memset / memcpy nodes
    rgb, d = _frame(53)
    ins["rgb"].copy_(torch.from_numpy(rgb)); ins["depth"].copy_(torch.from_numpy(d))
    g.replay()
    torch.cuda.synchronize()
    assert (_bits(out["depth"].cpu().numpy()) == _bits(im.depth(d, 5000.0))).all()


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _quaternion(R):
    """(qx, qy, qz, qw) of a rotation matrix with a positive trace (the room path turns by a few degrees)."""
    w = math.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2]) / 2.0
    return (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w


def test_tum_directory_round_trip_and_a_short_slam_run(native_lib, tmp_path):
    from PIL import Image
    from monogs_amd.dataset import dataset_frames, load_dataset
    from monogs_amd.sequences import make_room_sequence
    from monogs_amd.slam_harness import run_slam
    k = dict(fx=535.4 / 8, fy=539.2 / 8, cx=320.1 / 8, cy=247.6 / 8, W=80, H=60)
    src, _ = make_room_sequence(12, k, device=DEV)
    os.makedirs(tmp_path / "rgb"), os.makedirs(tmp_path / "depth")
    lists = {n: ["# header", "# header", "# header"] for n in ("rgb", "depth", "groundtruth")}
    written = []
    for i, f in enumerate(src):
        t = 100.0 + 0.04 * i
        rgb8 = (f.rgb.permute(1, 2, 0).cpu().double().numpy() * 255.0).round().clip(0, 255).astype(np.uint8)
        d16 = (f.depth.cpu().double().numpy() * 5000.0).round().clip(0, 65535).astype(np.uint16)
        written.append((rgb8, d16))
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
    ds = load_dataset(dict(Dataset=dict(type="tum", dataset_path=str(tmp_path), Calibration=cal)), device=DEV)
    assert len(ds) == 12
    item = ds[3]
    assert item["pose"].dtype == torch.float64 and item["pose"].shape == (4, 4) and item["segmentation"] is None
    assert item["mask"].dtype == item["grad_mask"].dtype == torch.bool and bool(item["mask"].all())
    frames, intr = dataset_frames(ds, 12, device=DEV)
    assert len(frames) == 12 and (intr.width, intr.height) == (80, 60)
    for f, s, (rgb8, d16) in zip(frames, src, written):
        assert (f.R_gt - s.R_gt).abs().max() <= 1e-6 and (f.T_gt - s.T_gt).abs().max() <= 1e-6
        # what the files hold comes back exactly ...
        assert (_bits(f.depth.cpu().numpy()) == _bits(im.depth(d16, 5000.0))).all()
        assert (_bits(f.rgb.cpu().numpy()) == _bits(im.colour(rgb8))).all()
        # ... so the distance to the source is the quantisation of the file format: half a step, plus the rounding of the
        # quotient to float32 (half an ulp of the largest depth, 2^-24 relative), both compared in float64
        err_d = (f.depth.double() - s.depth.double()).abs().max().item()
        err_c = (f.rgb.double() - s.rgb.double()).abs().max().item()
        assert err_d <= 0.5 / 5000 + 2.0 ** -24 * float(s.depth.max()), err_d
        assert err_c <= 0.5 / 255 + 1e-7, err_c
        assert f.mask.dtype == torch.bool and f.grad_mask.dtype == torch.bool and f.grad_mask.shape == (60, 80)
    r = run_slam(sequence=(frames, intr), tracking_itr_num=4, mapping_itr_num=4, init_itr_num=20, window_size=4, kf_interval=2)
    assert r["frames"] == 12 and r["width"] == 80
    assert r["config"]["tracking_itr_num"] == 4 and r["config"]["mapping_itr_num"] == 4
    for key in ("tracking_fps", "tracking_iters_per_s", "mapping_iters_per_s"):
        assert math.isfinite(r[key]) and r[key] > 0, (key, r[key])
