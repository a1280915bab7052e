"""The map's object layer (``GaussianMap(nr_objects=K)``): a row of object scores per Gaussian, one-hot from the segment id of the
pixel it was back-projected from, carried through clone / split / prune exactly as the reference carries ``_obj_prob``
(gaussian_splatting/scene/gaussian_model.py:693,764,808,855), and rendered per pixel by ``render_features``.
Run on the MI355X box: pytest -m gpu."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_OBJ = 6


def _build(nr_objects, n=2000, seed=0):
    """A map of n Gaussians whose first colour channel holds the object id: colours travel through the surgery exactly as the
    object rows must.  Half the scales lie below percent_dense x extent (clone candidates), half above (split candidates)."""
    from monogs_amd.gaussian_map import GaussianMap
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, K_OBJ, (n,), generator=g)
    rgb = torch.rand(n, 3, generator=g)
    rgb[:, 0] = ids.float()
    scaling = torch.where(torch.rand(n, 1, generator=g) < 0.5, torch.tensor(0.005), torch.tensor(0.05)).log()
    q = torch.randn(n, 4, generator=g)
    gmap = GaussianMap(DEV, nr_objects=nr_objects)
    gmap.densification_postfix(torch.randn(n, 3, generator=g).to(DEV), rgb.to(DEV), torch.randn(n, 1, generator=g).to(DEV),
                               scaling.to(DEV), q.to(DEV), new_obj_prob=_rows(ids) if nr_objects else None)
    return gmap


def _rows(ids):
    return torch.nn.functional.one_hot(ids.long(), K_OBJ).float().to(DEV)


def _surgery(gmap):
    """postfix, clone, split, prune with hand-made gradients and masks; yields (step, map size before) after every step."""
    g = torch.Generator().manual_seed(1)
    n = 300
    ids = torch.randint(0, K_OBJ, (n,), generator=g)
    rgb = torch.rand(n, 3, generator=g)
    rgb[:, 0] = ids.float()
    n0 = len(gmap)
    gmap.densification_postfix(torch.randn(n, 3, generator=g).to(DEV), rgb.to(DEV), torch.zeros(n, 1, device=DEV),
                               torch.full((n, 1), 0.005, device=DEV).log(), torch.randn(n, 4, generator=g).to(DEV),
                               new_obj_prob=_rows(ids) if gmap.nr_objects else None)
    yield "postfix", n0
    extent, thr = 1.0, 0.5                                  # percent_dense x extent = 0.01: between the two scales
    n0 = len(gmap)
    grads = (torch.rand(n0, 1, generator=g) < 0.4).float().to(DEV)      # 40 % of the Gaussians above the threshold
    gmap.densify_and_clone(grads, thr, extent)
    yield "clone", n0
    n0 = len(gmap)
    grads = (torch.rand(n0, 1, generator=g) < 0.3).float().to(DEV)
    gmap.densify_and_split(grads, thr, extent, generator=torch.Generator(device=DEV).manual_seed(5))
    yield "split", n0
    n0 = len(gmap)
    gmap.prune_points((torch.rand(n0, generator=g) < 0.25).to(DEV))
    yield "prune", n0


def test_surgery_carries_the_object_rows(native_lib):
    gmap = _build(K_OBJ)
    assert gmap._obj_prob.dtype == torch.float32 and not gmap._obj_prob.requires_grad
    assert all(p is not gmap._obj_prob for grp in (gmap.params(),) for p in grp)          # not an optimised parameter
    sizes = {}
    for step, n0 in _surgery(gmap):
        P = len(gmap)
        sizes[step] = (n0, P)
        o = gmap._obj_prob
        assert o.shape == (P, K_OBJ), step
        assert torch.equal(o.argmax(1), gmap._rgb[:, 0].detach().long()), step
        assert ((o == 0) | (o == 1)).all() and (o.sum(1) == 1).all(), step               # every row one-hot
        assert torch.allclose(gmap.get_obj_prob.sum(1), torch.ones(P, device=DEV), atol=1e-6), step
        assert not o.requires_grad
    # every step selected some Gaussians and left others
    assert sizes["postfix"] == (2000, 2300)
    assert 0 < sizes["clone"][1] - sizes["clone"][0] < sizes["clone"][0]
    assert sizes["split"][1] != sizes["split"][0] and sizes["split"][1] - sizes["split"][0] < sizes["split"][0]
    assert 0 < sizes["prune"][0] - sizes["prune"][1] < sizes["prune"][0]
    from monogs_amd.gaussian_map import object_colors, object_labels
    assert torch.equal(object_labels(gmap), gmap._rgb[:, 0].detach().long())
    palette = torch.rand(K_OBJ, 3, device=DEV)
    assert torch.equal(object_colors(gmap, palette), palette[gmap._rgb[:, 0].detach().long()])
    with pytest.raises(ValueError, match="new_obj_prob"):
        gmap.densification_postfix(*[torch.zeros(2, c, device=DEV) for c in (3, 3, 1, 1, 4)])


def test_map_without_object_layer_is_unchanged(native_lib):
    a, b = _build(None), _build(None)
    for (step, _), _ in zip(_surgery(a), _surgery(b)):
        assert a._obj_prob is None and b._obj_prob is None and a.nr_objects is None
        assert len(a) == len(b)
        for pa, pb in zip(a.params(), b.params()):
            assert torch.equal(pa, pb), step
        assert torch.equal(a.kf_idx, b.kf_idx) and torch.equal(a.nr_obs, b.nr_obs)
    with pytest.raises(AttributeError, match="no object layer"):
        a.get_obj_prob
    # the object layer changes nothing else: the same steps with it give the same parameters
    c = _build(K_OBJ)
    for _ in _surgery(c):
        pass
    for pa, pc in zip(a.params(), c.params()):
        assert torch.equal(pa, pc)


def _frame(H=60, W=80, seed=2):
    from monogs_amd import camera as cam
    g = torch.Generator().manual_seed(seed)
    Tcw = cam.se3_exp(torch.tensor([0.1, -0.2, 0.3, 0.05, 0.02, -0.04]))
    seg = torch.zeros(H, W, dtype=torch.int32)              # three regions: left third 0, upper right 2, lower right 5
    seg[: H // 2, W // 3:] = 2
    seg[H // 2:, W // 3:] = 5
    vp = types.SimpleNamespace(frame_idx=3, rgb=torch.rand(3, H, W, generator=g).to(DEV),
                               depth=(torch.rand(H, W, generator=g) * 3 + 0.5).to(DEV), segmentation=seg.to(DEV),
                               R=Tcw[:3, :3].contiguous().to(DEV), T=Tcw[:3, 3].contiguous().to(DEV),
                               exposure_a=torch.zeros(1, device=DEV), exposure_b=torch.zeros(1, device=DEV))
    return vp, types.SimpleNamespace(fx=70.0, fy=71.0, cx=40.3, cy=29.6), seg


def test_extend_from_frame_builds_one_hot_rows(native_lib):
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.keyframe import create_viewpoint_pcd
    vp, intr, seg = _frame()
    H, W = seg.shape
    pick = torch.randperm(H * W, generator=torch.Generator().manual_seed(9))        # every pixel is a candidate (depth > 0)
    pts, _, _, _, _, ids = create_viewpoint_pcd(vp, intr, init=True, random_indices=pick, downsample_factor=4)
    gmap = GaussianMap(DEV, nr_objects=K_OBJ)
    n_new = gmap.extend_from_frame(vp, intr, downsample=4, init=True, random_indices=pick)
    assert n_new == H * W // 4 == len(gmap) == ids.numel()
    assert torch.equal(gmap._xyz.detach(), pts)
    o = gmap._obj_prob
    assert o.shape == (n_new, K_OBJ) and ((o == 0) | (o == 1)).all() and (o.sum(1) == 1).all()
    assert torch.equal(o.argmax(1), ids.long())
    # and the ids are those of the pixels the points came from: candidates are numbered x outer, y inner
    px = pick[:n_new]
    assert torch.equal(ids.cpu().long(), seg[px % H, px // H].long())
    assert set(ids.cpu().tolist()) == {0, 2, 5}
    # a frame without segmentation: id 0 everywhere
    plain = types.SimpleNamespace(**{k: v for k, v in vars(vp).items() if k != "segmentation"})
    g0 = GaussianMap(DEV, nr_objects=K_OBJ)
    g0.extend_from_frame(plain, intr, downsample=4, init=True)
    assert (g0._obj_prob[:, 0] == 1).all() and (g0._obj_prob[:, 1:] == 0).all()
    # an id the map has no column for
    small = GaussianMap(DEV, nr_objects=5)
    with pytest.raises(ValueError, match="segmentation id 5"):
        small.extend_from_frame(vp, intr, downsample=4, init=True)
    assert len(small) == 0
    with pytest.raises(ValueError, match="1..256"):
        GaussianMap(DEV, nr_objects=257)


ROOM = dict(n_frames=12, intrinsics=dict(fx=535.4 / 4, fy=539.2 / 4, cx=320.1 / 4, cy=247.6 / 4, W=160, H=120),
            tracking_itr_num=100, mapping_itr_num=60, init_itr_num=600, window_size=4, kf_interval=2, scene="room")


def test_object_map_end_to_end(native_lib):
    """run_slam on the ray-cast room with its surface ids as segmentation; the per-pixel labels rendered from the map at the
    last keyframe must beat the always-guess-the-majority answer, computed here from the ground truth.
    Measured on the MI355X: accuracy 0.96 on every pixel of the frame against a majority share of 0.49 (11 surfaces in view)."""
    from monogs_amd import render_features
    from monogs_amd.mapping import render_map
    from monogs_amd.sequences import ROOM_SURFACES, make_room_sequence
    from monogs_amd.slam_harness import run_slam
    r = run_slam(nr_objects=ROOM_SURFACES, **ROOM)
    gmap, frames, intr = r["map"], r["frame_list"], r["intr"]
    assert gmap._obj_prob.shape == (len(gmap), ROOM_SURFACES) and len(gmap) == r["gaussians"]
    vp = frames[10]                                        # the last keyframe (every second frame is one)
    pkg = render_map(vp, intr, gmap, torch.zeros(3, device=DEV))
    feat, labels = render_features(pkg["render"], gmap.get_obj_prob, want_labels=True)
    assert feat.shape == (ROOM_SURFACES, 120, 160)
    gt = vp.segmentation.long()
    seen = labels >= 0
    assert seen.float().mean() > 0.5
    acc = (labels.long()[seen] == gt[seen]).float().mean().item()
    majority = torch.bincount(gt.reshape(-1), minlength=ROOM_SURFACES).max().item() / gt.numel()
    print(f"label accuracy at the last keyframe: {acc:.4f} on {seen.float().mean().item():.3f} of the pixels; "
          f"majority share {majority:.4f}; {int(gt.unique().numel())} surfaces in view")
    assert acc > majority
    # The same run without the layer: the parent's result keys, its frames and first map, and the same trajectory and map as far
    # as two runs of one sequence can agree.  They are not bit-identical: the order of the blend backward's float atomics differs,
    # Adam turns the last bits of a small gradient into steps of the size of the learning rate, and the keyframes after the
    # first add the few pixels that pass thresholds on the rendered opacity and depth error (50 x its median).  The iteration
    # counts are the smallest of five measured configurations at which this small room tracks at all (20 initialisation and 5
    # mapping iterations: both runs drift by 30 cm; 600 and 60, as here: ATE 8.5-10.2 mm, worst frame 11.5-14.5 mm over two plain
    # runs and one with the layer, 2424-2427 Gaussians; a run takes 0.8 s).  The bar is the one tests/test_gpu_slam.py derives for
    # two runs of one sequence: worst frame and ATE against the ground truth at most twice the other run's + 1.5 mm (15 % of the
    # ~1 cm the camera moves per frame), in both directions; the map sizes agree to 1 %.
    p = run_slam(**ROOM)
    assert not {"map", "frame_list", "intr"} & set(p)
    assert set(r) - set(p) == {"map", "frame_list", "intr"}
    plain, _ = make_room_sequence(2, ROOM["intrinsics"], device=DEV)
    for f, g in zip(plain, frames):                        # the segmentation rides along: same pixels, same depth
        assert torch.equal(f.rgb, g.rgb) and torch.equal(f.depth, g.depth) and not hasattr(f, "segmentation")
    assert r["surgery"]["gaussians_after_keyframe"][0] == p["surgery"]["gaussians_after_keyframe"][0] == 160 * 120 // 8
    assert r["keyframes"] == p["keyframes"] == 6 and r["window_sizes"] == p["window_sizes"] and r["tracked"] == p["tracked"] == 11
    worst = lambda x: max(x["position_error_m"])  # noqa: E731
    print(f"with / without the object layer: {r['gaussians']} / {p['gaussians']} Gaussians; worst frame {worst(r) * 1e3:.2f} / "
          f"{worst(p) * 1e3:.2f} mm, ATE {r['ate_rmse_m'] * 1e3:.2f} / {p['ate_rmse_m'] * 1e3:.2f} mm")
    assert abs(p["gaussians"] - r["gaussians"]) <= 0.01 * p["gaussians"]
    for a, b in ((r, p), (p, r)):
        assert worst(a) <= 2 * worst(b) + 1.5e-3 and a["ate_rmse_m"] <= 2 * b["ate_rmse_m"] + 1.5e-3
