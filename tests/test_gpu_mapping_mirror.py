"""``WindowMapper`` (monogs_amd/mapping.py) against the reference's ``optimize_map`` loop restated in plain PyTorch
(tests/mapping_mirror.py), teacher-forced: before every iteration the mirror is re-seeded from the mapper's state (raw
parameters, both Adam moments, per-tensor step counts, statistics, poses, exposures, pose-optimiser state), so every
iteration is a ONE-step comparison at a different optimiser state and every layer is held tightly instead of at the 2e-2 a
free-running (chaotic) Adam forces on tests/test_gpu_window.py (pytest -m gpu).

Every bar is exact equality or the bar an existing test applies to the same quantity, named where it is used."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("xyz", "f_dc", "opacity", "scaling", "rotation")
CAP = 1e-3          # share of Gaussians whose radius / touched flag may differ between two runs (_check_windows_agree)


@pytest.fixture(autouse=True)
def _release_device_state():
    """These tests run inside the pytest process; the window tests that follow start ranks of their own on the same device.
    Nothing of a finished test (captured graphs, their memory pool, cached blocks) stays behind for them."""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _setup(n_kf, window_size, use_graph=False, seed=7):
    """As ``_c4_setup`` of tests/test_gpu_window.py: keyframes at fr3_office slightly off the truth, the map from the first
    frame, the xyz schedule shortened (x 1e-3 over 300 iterations: 2.3 % per iteration) so that the rate moves visibly."""
    from monogs_amd import camera as cam
    from monogs_amd.gaussian_map import GaussianMap, REFERENCE_LR_SCHEDULE
    from monogs_amd.mapping import WindowMapper
    from monogs_amd.slam_harness import make_sequence
    frames, intr = make_sequence(n_kf, "fr3_office", n_gaussians=20000, device=DEV)
    for i, vp in enumerate(frames):
        d = cam.se3_exp(torch.tensor([0.002 * i, -0.001 * i, 0.0, 0.0, 0.0005 * i, 0.0], device=DEV))
        Tm = torch.eye(4, device=DEV)
        Tm[:3, :3], Tm[:3, 3] = vp.R_gt, vp.T_gt
        Tn = d @ Tm
        vp.update_RT(Tn[:3, :3], Tn[:3, 3])
    gmap = GaussianMap(DEV)
    gmap.lr_schedule = dict(REFERENCE_LR_SCHEDULE, lr_init=gmap.lrs[0], lr_final=gmap.lrs[0] * 1e-3, max_steps=300)
    gmap.extend_from_frame(frames[0], intr, downsample=8, init=True, point_size=1.0)
    bg = torch.zeros(3, device=DEV)
    mapper = WindowMapper(gmap, intr, bg, window_size=window_size, use_graph=use_graph, seed=seed)      # a single rank
    mapper.keep_reduced_grads = True
    return frames, intr, gmap, mapper, bg


def _mirror_of(mapper, gmap, intr, bg):
    from mapping_mirror import MirrorWindow
    m = MirrorWindow(intr, bg, mapper.window_size, seed=mapper.seed, pose_lrs=mapper.lrs, lr_schedule=gmap.lr_schedule)
    for k in ("gaussian_update_every", "gaussian_update_offset", "gaussian_th", "gaussian_extent", "gaussian_reset",
              "size_threshold", "densify_grad_threshold"):
        setattr(m, k, getattr(mapper, k))
    return m


def _reseed(mirror, mapper, gmap, frames, adopt_schedule=False):
    """The mirror takes the mapper's state.  Its iteration count and its xyz rate are its OWN bookkeeping (``expon_lr`` after
    every step) unless ``adopt_schedule``: a schedule that runs early or late in the mapper must show."""
    opt = gmap.optimizer
    lrs = list(opt.lrs)
    if mirror.opt is not None and not adopt_schedule:
        lrs[0] = mirror.group("xyz")["lr"]
    if adopt_schedule:
        mirror.nr_iters, mirror.first_time_pruned = mapper.nr_iters, mapper.first_time_pruned
    mirror.load_map(gmap.params(), opt.exp_avg, opt.exp_avg_sq, opt.t_dev.tolist(), lrs, gmap.xyz_gradient_accum, gmap.denom,
                    gmap.max_radii_2d, gmap.kf_idx, gmap.nr_obs)
    states = []
    for vp in frames:
        po = mapper._pose_opt.get(id(vp))
        states.append(None if po is None else (po.m, po.v, int(po.t_dev)))
    mirror.load_keyframes(frames, pose_states=states)


def _upstream(mapper):
    """What the mapper's fused loss handed to the rasteriser's backward in its last iteration, per keyframe."""
    return [(lg.d_render, lg.d_depth, lg.d_exposure_a, lg.d_exposure_b) for lg in mapper._plan.lgs]


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _like_for_like(a, b, tag):
    """test_two_rank_window_matches_single_process item (2): only the summation order differs between the two sides."""
    d, n = (a.double() - b.double()).norm().item(), b.double().norm().item()
    assert d <= 1e-5 * n + 1e-7, (tag, d, n)                # measured: gradients and accumulated norms <= 1.2 % of this bar
    return d / (1e-5 * n + 1e-7)


def _check_gradients(mapper, mirror, tag, bar):
    """xyz, rgb, opacity, scaling (the rotation gradient of an isotropic map is rounding noise on both sides)."""
    worst = 0.0
    for n, got, ref in list(zip(NAMES, mapper.last_grads, mirror.autograd_grads))[:4]:
        if got is None:                     # (an opacity reset replaced the tensor: no gradient, no step)
            assert n == "opacity", (tag, n)
            continue
        assert ref.abs().max() > 0, (tag, n)
        if bar == "torch loss":
            # test_c2_100k_mapping_loss_gradients: fused loss + HIP backward against torch loss + autograd, relative L2 <= 1e-3
            r = _rel(got, ref)                                  # measured <= 2.3e-5
            assert r < 1e-3, (tag, n, r)
            worst = max(worst, r / 1e-3)
        else:
            worst = max(worst, _like_for_like(got, ref, (tag, n)))
    return worst


def _check_statistics(mapper, gmap, mirror, pkgs, radii, touched, tag):
    """denom / max_radii_2d / visibility EQUAL wherever the two sides' radii and touched flags agree, the accumulated norms at
    the like-for-like bar; the share of Gaussians on which the two sides disagree is capped."""
    P = len(gmap)
    agree = torch.ones(P, dtype=torch.bool, device=DEV)
    for pkg, r, t in zip(pkgs, radii, touched):
        agree &= (pkg["radii"] == r) & ((pkg["n_touched"] > 0) == (t > 0))
    off = int((~agree).sum())
    assert off <= CAP * P, (tag, off, P)                        # measured: 0 of 38 390 in every iteration
    assert torch.equal(gmap.denom[agree], mirror.denom[agree]), tag
    assert torch.equal(gmap.max_radii_2d[agree], mirror.max_radii_2d[agree]), tag
    assert sorted(mapper.occ_aware_visibility) == sorted(mirror.occ_aware_visibility), tag
    for kf, vis in mirror.occ_aware_visibility.items():
        assert torch.equal(mapper.occ_aware_visibility[kf][agree], vis[agree]) and bool(vis.any()), (tag, kf)
    assert float(mirror.denom.max()) > 0 and float(mirror.max_radii_2d.max()) > 0
    return off, _like_for_like(gmap.xyz_gradient_accum[agree], mirror.xyz_gradient_accum[agree], (tag, "xyz_gradient_accum")), agree


def _check_optimizer(gmap, mirror, tag):
    """Parameters, both moments and the step counts of all five tensors at the bars of test_adam_state_surgery_matches_torch."""
    opt = gmap.optimizer
    for i, n in enumerate(NAMES):
        pa, pb, st = gmap.params()[i], mirror.params()[i], mirror.state(n)
        assert pa.shape == pb.shape, (tag, n)
        assert torch.allclose(pa, pb, rtol=1e-5, atol=3e-6), (tag, n, float((pa - pb).abs().max()))
        assert torch.allclose(opt.exp_avg[i], st["exp_avg"], rtol=1e-5, atol=1e-7), (tag, n)
        assert torch.allclose(opt.exp_avg_sq[i], st["exp_avg_sq"], rtol=1e-5, atol=1e-9), (tag, n)
        assert int(opt.t_dev[i]) == int(st["step"]), (tag, n, opt.t_dev.tolist())


def _check_poses(frames, mirror, frame0, tag):
    """test_pose_step_matches_adam_plus_update_pose: 2e-6 on R / T, 1e-6 on the exposures; frame 0 is the gauge."""
    worst = 0.0
    for f, v in zip(frames, mirror.vps):
        if f.frame_idx == 0:
            assert torch.equal(f.R, frame0[0]) and torch.equal(f.T, frame0[1]), tag
            assert torch.equal(f.exposure_a.data, frame0[2]) and torch.equal(f.exposure_b.data, frame0[3]), tag
            continue
        # (measured: <= 6 % of either bar)
        assert torch.allclose(f.R, v.R, atol=2e-6) and torch.allclose(f.T, v.T, atol=2e-6), (tag, f.frame_idx, (f.T - v.T).abs().max())
        assert torch.allclose(f.exposure_a, v.exposure_a, atol=1e-6) and torch.allclose(f.exposure_b, v.exposure_b, atol=1e-6), (tag, f.frame_idx)
        assert f.cam_rot_delta.abs().max() == 0 and f.cam_trans_delta.abs().max() == 0, tag
        worst = max(worst, float((f.R - v.R).abs().max()) / 2e-6, float((f.T - v.T).abs().max()) / 2e-6,
                    float((f.exposure_a - v.exposure_a).detach().abs().max()) / 1e-6,
                    float((f.exposure_b - v.exposure_b).detach().abs().max()) / 1e-6)
    return worst


def _frame0(frames):
    f = next(f for f in frames if f.frame_idx == 0)
    return [t.detach().clone() for t in (f.R, f.T, f.exposure_a, f.exposure_b)]


def _poses(frames):
    return [(v.R.detach().cpu().clone(), v.T.detach().cpu().clone(), v.exposure_a.data.cpu().clone(), v.exposure_b.data.cpu().clone())
            for v in frames]


# ---- (a) - (d), (f): twelve teacher-forced iterations, opacity resets on iterations 5 and 10 -----------------------------
def test_window_iteration_matches_the_reference_loop_step_for_step(native_lib):
    from monogs_amd.gaussian_optim import activate, expon_lr
    from monogs_amd.renderer import render
    iters = 12
    frames, intr, gmap, mapper, bg = _setup(4, 4)
    mapper.gaussian_reset = 5
    mirror, plain = _mirror_of(mapper, gmap, intr, bg), _mirror_of(mapper, gmap, intr, bg)
    P = len(gmap)
    assert P > 3000

    # (b), precondition: the cap on disagreeing radii is met by the two activation codes ALONE on this scene (expf in the
    # fused launch may round differently from torch.exp, which can move a radius across an integer)
    _reseed(mirror, mapper, gmap, frames)
    with torch.no_grad():
        rot, scales3, opac = activate(gmap._rotation.detach(), gmap._scaling.detach(), gmap._opacity.detach())
        flips = torch.zeros(P, dtype=torch.bool, device=DEV)
        for vp in mirror.vps:
            a = render(vp, intr, gmap._xyz.detach(), rot, scales3, opac, gmap._rgb.detach(), bg)
            b = render(vp, intr, gmap._xyz.detach(), torch.nn.functional.normalize(gmap._rotation.detach()),
                       torch.exp(gmap._scaling.detach()), torch.sigmoid(gmap._opacity.detach()), gmap._rgb.detach(), bg)
            flips |= (a["radii"] != b["radii"]) | ((a["n_touched"] > 0) != (b["n_touched"] > 0))
    print(f"radii / touched flags that differ between activate() and the torch activations: {int(flips.sum())} of {P}")
    assert int(flips.sum()) < CAP * P                             # measured: 0

    worst = dict(torch_loss=0.0, like=0.0, accum=0.0, pose=0.0, off=0)
    for it in range(1, iters + 1):
        _reseed(mirror, mapper, gmap, frames)
        frame0, poses_before = _frame0(frames), _poses(frames)
        reset = it % 5 == 0
        if it in (1, 6, 12):
            _reseed(plain, mapper, gmap, frames, adopt_schedule=True)
        before_opacity, steps_before = gmap._opacity.detach().clone(), gmap.optimizer.t_dev.tolist()
        assert mapper.optimize_map(frames, iters=1) == reset
        p = mapper._plan
        # (a) the gradients after the bucket and the explicit activation backward: against the plain loop (torch loss) ...
        if it in (1, 6, 12):
            plain.forward_backward()
            worst["torch_loss"] = max(worst["torch_loss"], _check_gradients(mapper, plain, (it, "torch loss"), "torch loss"))
        # ... and like for like (the mirror's renders pulled back through the mapper's own upstream tensors)
        pkgs = mirror.forward_backward(upstream=_upstream(mapper))
        worst["like"] = max(worst["like"], _check_gradients(mapper, mirror, (it, "like for like"), "like"))
        # (b) visibility and statistics, every iteration (after 1 and after several)
        mirror.visibility(pkgs)
        mirror.statistics(pkgs)
        off, acc, agree = _check_statistics(mapper, gmap, mirror, pkgs, p.radii, p.n_touched, it)
        worst["accum"], worst["off"] = max(worst["accum"], acc), max(worst["off"], off)
        # (c) the mapper's own gradients through torch.optim.Adam at the rate the mirror's schedule says applies to this step
        assert mirror.surgery_and_steps(pkgs, gaussian_grads=mapper.last_grads) == reset
        assert mirror.nr_iters == mapper.nr_iters == it
        _check_optimizer(gmap, mirror, it)
        want = [s + 1 for s in steps_before]
        if reset:
            # (f) the opacity tensor is replaced, takes no step and keeps its count; its moments restart from zero; the
            # reset values are exact wherever the visible union is (where the radii agree)
            want[2] -= 1
            assert mapper.last_grads[2] is None and all(g is not None for i, g in enumerate(mapper.last_grads) if i != 2)
            assert torch.equal(gmap._opacity.detach()[agree], mirror.params()[2].detach()[agree]), it
            assert not torch.equal(gmap._opacity.detach(), before_opacity)
            assert float(gmap.optimizer.exp_avg[2].abs().max()) == 0 and float(gmap.optimizer.exp_avg_sq[2].abs().max()) == 0
        assert gmap.optimizer.t_dev.tolist() == want, (it, gmap.optimizer.t_dev.tolist(), want)
        # (d) poses and exposures: Adam + retract_pose
        worst["pose"] = max(worst["pose"], _check_poses(frames, mirror, frame0, it))
        assert all(not torch.equal(f.T, b[1].to(DEV)) for f, b in zip(frames[1:], poses_before[1:])), it       # they did move
    lr = expon_lr(iters, **gmap.lr_schedule)
    assert abs(gmap.optimizer.lrs[0] - lr) <= 1e-6 * lr            # update_learning_rate(nr_iters), the bar of test_captured_...
    assert abs(mirror.group("xyz")["lr"] - lr) <= 1e-12 * lr and lr < 0.8 * gmap.lrs[0]
    print("worst / bar over 12 iterations: gradients vs torch loss %.3g (bar 1e-3), like for like %.3g (1e-5 |b| + 1e-7), "
          "xyz_gradient_accum %.3g (same), poses %.3g (2e-6 / 1e-6); at most %d of %d Gaussians disagree on a radius"
          % (worst["torch_loss"], worst["like"], worst["accum"], worst["pose"], worst["off"], P))


# ---- (e) the same iterations replayed from a hipGraph ------------------------------------------------------------------
def _window_result(gmap, mapper, frames, before):
    return dict(params=[p.detach().cpu() for p in gmap.params()], before=before, P=len(gmap), nr_iters=mapper.nr_iters,
                stats=(gmap.xyz_gradient_accum.cpu(), gmap.denom.cpu(), gmap.max_radii_2d.cpu()),
                vis={k: v.cpu() for k, v in mapper.occ_aware_visibility.items()}, lrs=list(gmap.optimizer.lrs),
                steps=gmap.optimizer.t_dev.cpu(), poses=_poses(frames))


def test_captured_iterations_match_eager_which_matches_the_mirror(native_lib):
    """The eager mapper free-runs 12 iterations; the mirror, seeded once, takes the eager mapper's gradients through
    torch.optim.Adam and its own schedule over the whole span and must end where the mapper ends ((c)'s bars, as
    test_gaussian_adam_matches_torch_adam holds them over 12 steps).  The captured run (one eager iteration, one capture,
    11 replays) is then held against the eager one at the bars of ``_check_windows_agree``."""
    from test_gpu_window import _check_windows_agree
    iters = 12
    frames, intr, gmap, mapper, bg = _setup(4, 4)
    mapper.map_surgery = False
    mirror = _mirror_of(mapper, gmap, intr, bg)
    _reseed(mirror, mapper, gmap, frames)
    before = [p.detach().cpu().clone() for p in gmap.params()]
    for it in range(iters):
        mapper.optimize_map(frames, iters=1)
        mirror.optimizer_step_only(mapper.last_grads)
    _check_optimizer(gmap, mirror, "eager span")
    eager = _window_result(gmap, mapper, frames, before)
    assert mapper.stats["replays"] == 0 and mapper.stats["eager_iters"] == iters

    frames, intr, gmap, mapper, bg = _setup(4, 4, use_graph=True)
    mapper.map_surgery = False
    mapper.optimize_map(frames, iters=iters)
    assert mapper.stats["captures"] == 1 and mapper.stats["replays"] == iters - 1 and mapper.stats["eager_iters"] == 1
    graph = _window_result(gmap, mapper, frames, before)
    mapper._drop_plan()                                  # (the captured graph goes with the test)
    _check_windows_agree(graph, eager, 4, iters)


def test_recaptured_iterations_match_eager_and_forget_the_dropped_captures(native_lib):
    """``max_replays_per_capture = 3`` over 12 iterations: eager, capture, 3 replays -- three times over.  The result is held
    against the all-eager run at the bars of ``_check_windows_agree``; the status words of the two captures that were dropped on
    the way are gone from the ledger, the live plan's handle holds one word per forward its graph captured (single rank: one
    graph, one forward per window keyframe), and ``_drop_plan()`` leaves none."""
    from test_gpu_window import _check_windows_agree
    from monogs_amd import rasterizer as R
    iters = 12
    frames, intr, gmap, mapper, bg = _setup(2, 2)
    mapper.map_surgery = False
    before = [p.detach().cpu().clone() for p in gmap.params()]
    mapper.optimize_map(frames, iters=iters)
    eager = _window_result(gmap, mapper, frames, before)
    assert mapper.stats["replays"] == 0 and mapper.stats["eager_iters"] == iters
    mapper._drop_plan()
    R.check_overflow()
    R.clear_graph_flags()                                # (whatever earlier tests of this process left behind)

    frames, intr, gmap, mapper, bg = _setup(2, 2, use_graph=True)
    mapper.map_surgery = False
    mapper.max_replays_per_capture = 3
    mapper.optimize_map(frames, iters=iters)
    assert mapper.stats["captures"] == 3 and mapper.stats["replays"] == 9 and mapper.stats["eager_iters"] == 3, mapper.stats
    graph = _window_result(gmap, mapper, frames, before)
    p = mapper._plan
    assert p.graphs is not None and len(p.graphs) == 1
    assert len(p.graph_flags) == len(p.vps) == 2
    assert R._ledger.captured_words() == p.graph_flags.words       # nothing of the two dropped captures
    assert not R.check_overflow()
    mapper._drop_plan()
    assert R._ledger.captured_words() == []
    _check_windows_agree(graph, eager, 2, iters)


# ---- (g) the densify iteration -----------------------------------------------------------------------------------------
def test_densify_iteration_picks_the_reference_gaussians(native_lib):
    from monogs_amd.gaussian_optim import expon_lr
    frames, intr, gmap, mapper, bg = _setup(4, 4)
    mapper.gaussian_update_every, mapper.gaussian_update_offset = 4, 0           # densify_and_prune on iteration 4
    mapper.gaussian_th = 0.05                    # (0.7 would prune the whole young map: opacities start at 0.5)
    gmap.surgery_log = []
    mapper.optimize_map(frames, iters=3)
    assert len(gmap.surgery_log) == 0
    # The clone / split decision sits on `grads >= threshold` and the two sides' norms differ in their last digits: the
    # threshold comes from the MIRROR's statistics alone, at the midpoint of the widest gap between consecutive sorted values
    # in the middle half of the distribution, and that gap must be >= 100 x the (b) bar x the threshold
    probe = _mirror_of(mapper, gmap, intr, bg)
    _reseed(probe, mapper, gmap, frames, adopt_schedule=True)
    pkgs = probe.forward_backward()
    probe.visibility(pkgs)
    probe.statistics(pkgs)
    g = (probe.xyz_gradient_accum / probe.denom).squeeze(1)
    g = torch.sort(g[torch.isfinite(g)]).values
    mid = g[g.numel() // 4: 3 * g.numel() // 4]
    gaps = mid[1:] - mid[:-1]
    j = int(torch.argmax(gaps))
    thr = 0.5 * (float(mid[j]) + float(mid[j + 1]))
    print(f"densify threshold {thr:.6g}, widest gap / threshold = {float(gaps[j]) / thr:.3g} (needs >= 1e-3)")
    assert float(gaps[j]) >= 100 * 1e-5 * thr                     # measured: gap = 1.43e-3 x threshold (threshold 1.74e-5)
    mapper.densify_grad_threshold = thr

    mirror = _mirror_of(mapper, gmap, intr, bg)
    _reseed(mirror, mapper, gmap, frames, adopt_schedule=True)
    frame0, steps, poses_before = _frame0(frames), gmap.optimizer.t_dev.tolist(), _poses(frames)
    n0 = len(gmap)
    assert mapper.optimize_map(frames, iters=1) is True
    split, pkgs = mirror.iterate(upstream=_upstream(mapper))
    assert split is True and mirror.nr_iters == mapper.nr_iters == 4
    log = gmap.surgery_log[-1]
    sizes = [log["before"], log["before"] + log["cloned"], log["before"] + log["cloned"] + log["split_net"], log["after"]]
    print(f"map sizes before / after clone / after split / after prune: {sizes}")
    assert sizes == mirror.surgery_log[-1] and sizes[0] == n0 and len(gmap) == sizes[3]
    assert sizes[1] > sizes[0] or sizes[2] != sizes[1]                     # something was cloned or split
    for n, a, b in zip(NAMES, gmap.params(), mirror.params()):
        assert torch.equal(a.detach(), b.detach()), n                      # kept and new rows of all five tensors
        assert a.is_leaf and a.requires_grad and a.grad is None
    assert torch.equal(gmap.kf_idx, mirror.kf_idx) and torch.equal(gmap.nr_obs, mirror.nr_obs)
    for a, b in ((gmap.xyz_gradient_accum, mirror.xyz_gradient_accum), (gmap.denom, mirror.denom), (gmap.max_radii_2d, mirror.max_radii_2d)):
        assert a.shape == b.shape and float(a.abs().max()) == 0 and float(b.abs().max()) == 0       # the zeroed statistics
    for i, n in enumerate(NAMES):
        st = mirror.state(n)
        assert torch.equal(gmap.optimizer.exp_avg[i], st["exp_avg"]) and torch.equal(gmap.optimizer.exp_avg_sq[i], st["exp_avg_sq"]), n
        assert int(gmap.optimizer.t_dev[i]) == int(st["step"]) == steps[i], n          # no tensor steps on that iteration
    n_new = sizes[3] - int((mirror.state("xyz")["exp_avg"].abs().sum(1) > 0).sum())
    assert n_new > 0 and all(g is None for g in mapper.last_grads)
    lr = expon_lr(4, **gmap.lr_schedule)                                               # the schedule and the poses still step
    assert abs(gmap.optimizer.lrs[0] - lr) <= 1e-6 * lr and abs(mirror.group("xyz")["lr"] - lr) <= 1e-12 * lr
    worst = _check_poses(frames, mirror, frame0, "densify")
    assert all(not torch.equal(f.T, b[1].to(DEV)) for f, b in zip(frames[1:], poses_before[1:]))
    print(f"poses after the densify iteration: worst / bar = {worst:.3g}")


# ---- (h) the pruning call ----------------------------------------------------------------------------------------------
def test_pruning_call_on_a_window_that_is_not_full_carries_its_gradients(native_lib):
    """``optimize_map(prune=True)`` steps nothing and leaves its gradients in ``.grad``; the next call's backward adds to them."""
    frames, intr, gmap, mapper, bg = _setup(3, 8)
    mapper.optimize_map(frames, iters=1)
    mirror = _mirror_of(mapper, gmap, intr, bg)
    _reseed(mirror, mapper, gmap, frames, adopt_schedule=True)
    frame0, steps = _frame0(frames), gmap.optimizer.t_dev.tolist()
    params = [p.detach().clone() for p in gmap.params()]
    assert mapper.optimize_map(frames, prune=True, iters=1) is False
    split, pkgs = mirror.iterate(prune=True, upstream=_upstream(mapper))
    assert gmap.optimizer.t_dev.tolist() == steps and all(torch.equal(a, b.detach()) for a, b in zip(params, gmap.params()))
    assert all(p.grad is not None for p in mirror.params()) and mirror.nr_iters == mapper.nr_iters == 2
    for kf, vis in mirror.occ_aware_visibility.items():
        assert (mapper.occ_aware_visibility[kf] != vis).float().mean() <= CAP and bool(vis.any())
    mapper.optimize_map(frames, iters=1)
    p = mapper._plan
    pkgs = mirror.forward_backward(upstream=_upstream(mapper))          # adds to what the pruning call left in .grad
    worst = _check_gradients(mapper, mirror, "after the pruning call", "like")
    single = [g.norm().item() for g in mapper.last_grads[:4]]
    mirror.visibility(pkgs)
    mirror.statistics(pkgs)
    off, acc, _ = _check_statistics(mapper, gmap, mirror, pkgs, p.radii, p.n_touched, "after the pruning call")
    mirror.surgery_and_steps(pkgs, gaussian_grads=mapper.last_grads)
    _check_optimizer(gmap, mirror, "after the pruning call")
    pose = _check_poses(frames, mirror, frame0, "after the pruning call")    # (the pose gradients of both backwards, too)
    mapper.optimize_map(frames, iters=1)                                 # a plain iteration again: about half the gradient
    for s, g in zip(single, mapper.last_grads[:4]):
        assert 1.6 < s / g.norm().item() < 2.4
    print(f"carried gradients: worst / bar = {worst:.3g}; xyz_gradient_accum {acc:.3g}; poses {pose:.3g}; {off} radii disagree")


def test_full_window_pruning_call_picks_the_reference_gaussians(native_lib):
    from monogs_amd import camera as cam
    frames, intr, gmap, mapper, bg = _setup(4, 4)
    P = len(gmap)
    gmap.kf_idx = (torch.arange(P, device=DEV) % 4).to(torch.int32)        # Gaussians born in every keyframe of the window
    mapper.optimize_map(frames, iters=2)
    mirror = _mirror_of(mapper, gmap, intr, bg)

    def prune_both(tag):
        """Both sides prune; returns the two prune masks.  ``max_radii_2d`` carries the row numbers through ``prune_points``
        (a per-Gaussian array the pruning call does not otherwise touch), which names the rows each side kept."""
        n = len(gmap)
        gmap.max_radii_2d = torch.arange(n, device=DEV, dtype=torch.float32)
        _reseed(mirror, mapper, gmap, frames, adopt_schedule=True)
        kf_idx = gmap.kf_idx.clone()
        assert mapper.optimize_map(frames, prune=True, iters=1) is False
        mirror.iterate(prune=True)
        masks = []
        for kept in (gmap.max_radii_2d, mirror.max_radii_2d):
            m = torch.ones(n, dtype=torch.bool, device=DEV)
            m[kept.long()] = False
            masks.append(m)
        differ = int((masks[0] != masks[1]).sum())
        print(f"{tag}: {int(masks[0].sum())} of {n} pruned, the masks differ on {differ}")
        assert differ <= CAP * n                                          # measured 0 (a touched flag may flip with the activations' rounding)
        assert mapper.first_time_pruned and mirror.first_time_pruned and mirror.nr_iters == mapper.nr_iters
        assert sorted(mapper.occ_aware_visibility) == sorted(mirror.occ_aware_visibility) == [0, 1, 2, 3]
        if differ == 0:
            assert len(gmap) == mirror.params()[0].shape[0] == n - int(masks[0].sum())
            assert torch.equal(gmap.max_radii_2d, mirror.max_radii_2d)
            for a, b in zip(gmap.params(), mirror.params()):
                assert torch.equal(a.detach(), b.detach())
            assert torch.equal(gmap.kf_idx, mirror.kf_idx) and torch.equal(gmap.nr_obs, mirror.nr_obs)
            for kf, vis in mirror.occ_aware_visibility.items():            # the re-indexed visibility
                got = mapper.occ_aware_visibility[kf]
                assert got.shape == vis.shape == (len(gmap),) and (got != vis).float().mean() <= CAP
            for i, n_ in enumerate(NAMES):
                assert torch.equal(gmap.optimizer.exp_avg[i], mirror.state(n_)["exp_avg"])
        return masks[0], kf_idx

    assert not mapper.first_time_pruned
    mask, kf_idx = prune_both("first full-window prune")
    assert 0 < int(mask.sum()) < P and bool(mask[kf_idx == 0].any())       # first time: Gaussians of every keyframe may go
    # a keyframe turns away, so that part of the map is seen by three keyframes only; the second prune may then drop only the
    # Gaussians of the three newest keyframes (kf_idx >= sorted(window, reverse=True)[2] = 1)
    f = frames[3]
    d = cam.se3_exp(torch.tensor([0.0, 0.0, 0.0, 0.0, 0.25, 0.0], device=DEV))
    Tm = torch.eye(4, device=DEV)
    Tm[:3, :3], Tm[:3, 3] = f.R, f.T
    Tn = d @ Tm
    f.update_RT(Tn[:3, :3], Tn[:3, 3])
    mapper.optimize_map(frames, iters=1)
    mask, kf_idx = prune_both("second full-window prune")
    assert int(mask.sum()) > 0 and not bool(mask[kf_idx == 0].any()) and bool(mask[kf_idx == 1].any())
    assert bool((gmap.nr_obs[gmap.kf_idx == 0] <= 3).any())                # the keyframe mask kept them, not their count
