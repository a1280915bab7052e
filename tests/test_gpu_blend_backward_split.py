"""The split blend backward (mgs_debug_set_option("blend_bwd_split", 1 | 2)): every quadrant's list is walked by two waves, the
positions [0, m) front to back -- T from the forward's own product, the colour behind from a prefix sum and the forward's finished
colour and depth images -- and [m, maxc) back to front as before.  Held against the unsplit walk (option 0) of the same build
with the bars tests/test_gpu_parity.py::test_c2_100k_mapping_loss_gradients applies against the oracle (`_check_grads` there):
relative L2 of every gradient tensor <= 1e-4, and elementwise |got - ref| <= 1e-3 |ref| + 1e-5 max|ref| for all but a 2e-4
fraction of the elements."""
import ctypes as C

import pytest
import torch

from monogs_amd.synthetic import make_scene, scene_settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L2_TOL, RTOL, ATOL_OF_MAX, MAX_OUTLIER_FRAC = 1e-4, 1e-3, 1e-5, 2e-4      # test_gpu_parity._check_grads


def _settings(sc):
    from monogs_amd.rasterizer import GaussianRasterizationSettings
    return scene_settings(sc, GaussianRasterizationSettings, device=DEV)


def _Split(lib, split, **knobs):
    """blend_bwd_split (and optionally the split's own knobs) for the duration of a block; the defaults afterwards."""
    from monogs_amd.debug import options
    return options(blend_bwd_split=split, **{"blend_bwd_split_" + k: v for k, v in knobs.items()})


def _grads(sc, pose_only=False, passes=1):
    """Forward + backward through the rasteriser; `passes` backwards through the one forward (the last one's gradients)."""
    from monogs_amd.rasterizer import GaussianRasterizer
    scales = sc.scales if sc.scales.shape[1] == 3 else sc.scales.repeat(1, 3)
    inp = dict(means3D=sc.means3D, opacities=sc.opacities, colors_precomp=sc.colors, scales=scales, rotations=sc.rotations)
    leaves = {k: (v.to(DEV).clone() if pose_only else v.to(DEV).clone().requires_grad_(True)) for k, v in inp.items()}
    theta = torch.zeros(3, device=DEV, requires_grad=True)
    rho = torch.zeros(3, device=DEV, requires_grad=True)
    m2 = torch.zeros_like(leaves["means3D"], requires_grad=not pose_only)
    out = GaussianRasterizer(_settings(sc))(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"],
                                            colors_precomp=leaves["colors_precomp"], scales=leaves["scales"],
                                            rotations=leaves["rotations"], theta=theta, rho=rho)
    images = [o.detach().clone() for o in (out[0], out[2], out[3])]
    loss = (out[0] * sc.grad_color.to(DEV)).sum() + (out[2] * sc.grad_depth.to(DEV)).sum()
    params = list(leaves.values()) + [m2] if not pose_only else []
    for i in range(passes):
        for p in params + [theta, rho]:
            p.grad = None
        loss.backward(retain_graph=i + 1 < passes)
    g = dict(theta=theta.grad.clone(), rho=rho.grad.clone())
    if not pose_only:
        g.update({k: v.grad.clone() for k, v in leaves.items()}, means2D=m2.grad.clone())
    return images, g


def _hold(got, ref, what):
    assert set(got) == set(ref)
    report = {}
    for k in ref:
        x, y = got[k].double(), ref[k].double()
        scale = y.abs().max().item()
        assert scale > 0, (what, k)
        rel = ((x - y).norm() / y.norm()).item()
        bad = ((x - y).abs() > RTOL * y.abs() + ATOL_OF_MAX * scale).float().mean().item()
        report[k] = (f"{rel:.2e}", f"{bad:.1e}")
        assert rel <= L2_TOL, (what, k, rel)
        assert bad <= MAX_OUTLIER_FRAC, (what, k, bad)
    print(what, report)


def _split_vs_unsplit(lib, sc, what, modes=(1, 2), **kw):
    with _Split(lib, 0):
        img0, ref = _grads(sc, **kw)
        assert lib.mgs_debug_last_backward_split() == 0
    for mode in modes:
        with _Split(lib, mode):
            img1, got = _grads(sc, **kw)
            assert lib.mgs_debug_last_backward_split() == 1
        for a, b in zip(img0, img1):
            assert torch.equal(a, b)                    # the forward is not touched
        _hold(got, ref, f"{what} [split {mode}]")
    return ref


@pytest.mark.parametrize("pose_only", [False, True])
@pytest.mark.parametrize("P,intr,seed", [(5000, "fr3_office", 0), (100000, "fr3_office", 1), (60000, "replica", 4)])
def test_split_matches_unsplit_on_the_parity_scenes(native_lib, P, intr, seed, pose_only):
    """The scenes of test_blend_backward_paths_agree, ten-sum and six-sum (pose-only) variant.  Replica's 680 rows end half
    way through a row of tiles: pixels outside the image in both walks."""
    _split_vs_unsplit(native_lib, make_scene(P, intr, seed=seed), f"{P} {intr}", pose_only=pose_only)


def test_short_lists_leave_the_front_wave_idle(native_lib):
    """2 000 Gaussians at VGA: no quadrant's walk reaches the shortest list that is split (four 64-instance steps), so m = 0
    everywhere, the front waves return at once and the back waves walk everything.  Also with the minimum raised above every
    list of a scene that is split by default."""
    _split_vs_unsplit(native_lib, make_scene(2000, "fr3_office", seed=3), "short lists")
    sc = make_scene(40000, "fr3_office", seed=9)
    with _Split(native_lib, 0):
        _, ref = _grads(sc)
    with _Split(native_lib, 1, min=1 << 20):
        _, got = _grads(sc)
    _hold(got, ref, "minimum above every list")


def test_uneven_split_points(native_lib):
    """The front walk's share at both ends of its range: m is clamped to [one step, all but one step]."""
    sc = make_scene(100000, "fr3_office", seed=1)
    with _Split(native_lib, 0):
        _, ref = _grads(sc)
    for frac in (1, 64, 255):
        with _Split(native_lib, 1, frac=frac):
            _, got = _grads(sc)
        _hold(got, ref, f"front share {frac}/256")


def test_opaque_scene_saturates_in_the_front_part(native_lib):
    """Nearly opaque splats: pixels saturate after a few contributors, so the walked depth (the quadrant's longest pixel) is
    set by a few pixels and most pixels of a quadrant have nothing behind m: back waves with almost every lane idle."""
    sc = make_scene(150000, "fr3_office", seed=21, mean_radius_px=10.0)
    sc = sc._replace(opacities=torch.full_like(sc.opacities, 0.97))
    _split_vs_unsplit(native_lib, sc, "opaque")


def test_empty_tiles_and_background(native_lib):
    """Gaussians bunched in the image centre (empty tiles all round) over a non-zero background: the background term of
    dL/dalpha is inside the front walk's prefix scalar, not a separate product."""
    sc = make_scene(60000, "fr3_office", seed=5, spread=0.45, bg=(0.3, 0.6, 0.9))
    _split_vs_unsplit(native_lib, sc, "empty tiles + background")


def test_lists_longer_than_1024(native_lib):
    """Large splats on the global-sort path: tiles of more than 1024 instances, walked from point_list."""
    from monogs_amd.debug import forward_tables
    sc = make_scene(12000, "fr3_office", seed=4, mean_radius_px=80.0)
    st = _settings(sc)
    assert native_lib.mgs_binning_path(12000, 640, 480) == 0
    t = forward_tables(st, sc.means3D.to(DEV), sc.opacities.to(DEV), colors_precomp=sc.colors.to(DEV),
                       scales=sc.scales.repeat(1, 3).to(DEV), rotations=sc.rotations.to(DEV))
    n = (t["ranges"][:, 1] - t["ranges"][:, 0]).long()
    assert int((n > 1024).sum()) > 0
    _split_vs_unsplit(native_lib, sc, "lists > 1024")


def test_per_tile_sorted_lists(native_lib):
    """Above 512 k Gaussians the blend forward sorts each tile's list itself and leaves it in point_list for the backward: the
    path of the flagship workload.  All eight tensors at the full bar, both launch orders.  The upstream gradient is COHERENT
    (a constant positive dL/dcolor and dL/ddepth) instead of the scene's uniform noise: under noise the pose gradient of
    600 k Gaussians is six sums that cancel to four digits, which no two float32 evaluations agree on elementwise (the float32
    oracle's own theta is then 8e-5 from float64's; tools/grad_accuracy.py has that case against float64)."""
    sc = make_scene(600000, "fr3_office", seed=2, mean_radius_px=3.0)
    H, W = sc.grad_depth.shape[1:]
    sc = sc._replace(grad_color=torch.full_like(sc.grad_color, 1.0 / (3 * H * W)), grad_depth=torch.full_like(sc.grad_depth, 1.0 / (H * W)))
    assert native_lib.mgs_binning_path(600000, 640, 480) == 1
    _split_vs_unsplit(native_lib, sc, "per-tile path")


def test_capacity_overflow(native_lib):
    """Capacity mode with too few slots: truncated lists, the overflow flag raised, and both walks agree on what was blended."""
    from monogs_amd import rasterizer as R
    sc = make_scene(20000, "fr3_office", seed=131)
    key = (20000, 640, 480)
    R.set_sync_free(False)
    _grads(sc)                                         # exact path: records the capacity hint
    try:
        full = R.capacity_hint(*key)
        res = {}
        for mode in (0, 1):
            R.reserve_capacity(*key, full // 2)
            R.set_sync_free(True, headroom=1.0)
            with _Split(native_lib, mode):
                res[mode] = _grads(sc)
            assert R.check_overflow()
        for a, b in zip(res[0][0], res[1][0]):
            assert torch.equal(a, b)
        _hold(res[1][1], res[0][1], "capacity overflow")
    finally:
        R.set_sync_free(False)
        R.forget_capacity(*key)


def test_second_backward_through_one_forward(native_lib):
    """The second backward (fresh scratch, cleared by a launch) of a split run against the second backward of an unsplit run."""
    sc = make_scene(30000, "fr3_office", seed=77)
    with _Split(native_lib, 0):
        _, ref = _grads(sc, passes=2)
    with _Split(native_lib, 1):
        _, got = _grads(sc, passes=2)
        assert native_lib.mgs_debug_last_backward_split() == 1
    _hold(got, ref, "second backward")


def test_without_the_forward_images_the_walk_is_unsplit(native_lib, monkeypatch):
    """mgs_backward with a NULL colour or depth pointer walks unsplit whatever the option says -- asserted on the launch itself
    (mgs_debug_last_backward_split) -- and its gradients are option 0's up to the order of the float atomics (the bar of
    test_second_backward_through_one_forward in test_gpu_features.py: 1e-5 relative L2; theta and rho, six sums over the map:
    the 1e-5 of test_blend_backward_paths_agree).  Two ways there: the rasteriser holds its output images weakly and passes NULL
    once the caller has dropped them (not an error); and a caller of the C ABI that passes only one of the two."""
    sc = make_scene(30000, "fr3_office", seed=8)

    def run(drop):
        from monogs_amd.rasterizer import GaussianRasterizer
        leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
        m, o, c, r, s = leaf(sc.means3D), leaf(sc.opacities), leaf(sc.colors), leaf(sc.rotations), leaf(sc.scales.repeat(1, 3))
        m2 = torch.zeros_like(m, requires_grad=True)
        th, rh = torch.zeros(3, device=DEV, requires_grad=True), torch.zeros(3, device=DEV, requires_grad=True)
        out = GaussianRasterizer(_settings(sc))(means3D=m, means2D=m2, opacities=o, colors_precomp=c, scales=s, rotations=r,
                                                theta=th, rho=rh)
        fn = out[0].grad_fn
        # (a product with a constant keeps the constant, not the image)
        loss = (out[0] * sc.grad_color.to(DEV)).sum() + (out[2] * sc.grad_depth.to(DEV)).sum()
        if drop:
            del out
            assert fn.out_ref() is None
        else:
            assert fn.out_ref() is not None
        loss.backward()
        return [t.grad.clone() for t in (m, o, c, r, s, m2, th, rh)]

    def same(got, ref):
        for a, b in zip(got, ref):
            assert b.abs().max() > 0
            assert ((a - b).norm() / b.norm()).item() < 1e-5

    with _Split(native_lib, 0):
        ref = run(False)
        assert native_lib.mgs_debug_last_backward_split() == 0
    with _Split(native_lib, 1):
        kept = run(False)
        assert native_lib.mgs_debug_last_backward_split() == 1          # (the images were there: split)
        got = run(True)
        assert native_lib.mgs_debug_last_backward_split() == 0
        same(got, ref)
        # the C ABI with ONE of the two pointers NULL (argument 16 = out_color, 17 = out_depth)
        real = native_lib.mgs_backward
        for null in (16, 17):
            monkeypatch.setattr(native_lib, "mgs_backward", lambda *a, _n=null: real(*a[:_n], None, *a[_n + 1:]), raising=False)
            got = run(False)
            monkeypatch.undo()
            assert native_lib.mgs_debug_last_backward_split() == 0, null
            same(got, ref)
    _hold(dict(zip("abcdefgh", kept)), dict(zip("abcdefgh", ref)), "kept images")


def test_option_values(native_lib):
    lib = native_lib
    for v in (0, 1, 2, -1):
        assert lib.mgs_debug_set_option(b"blend_bwd_split", C.c_int64(v)) == 0
    assert lib.mgs_debug_set_option(b"blend_bwd_split_min", -1) == 0 and lib.mgs_debug_set_option(b"blend_bwd_split_frac", -1) == 0
