"""``Refiner`` (monogs_amd/refinement.py) against the reference's ``Mapper.refinement`` loop restated in plain PyTorch
(tests/refinement_mirror.py), teacher-forced like tests/test_gpu_mapping_mirror.py, and its hipGraph mode against its eager
mode (pytest -m gpu).

Every bar is exact equality or the bar an existing test applies to the same quantity, named where it is used."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAPPER_ITERS = 3        # mapping iterations before the refinement: the mapper's schedule has moved, the refinement restarts it


@pytest.fixture(autouse=True)
def _release_device_state():
    """Nothing of a finished test (captured graphs, their memory pool, cached blocks) stays behind for the tests that follow."""
    yield
    import gc
    from monogs_amd import rasterizer
    rasterizer.clear_graph_flags()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _setup(**kw):
    """The setup of tests/test_gpu_mapping_mirror.py (three keyframes at fr3_office, the map from frame 0, the shortened xyz
    schedule), a few mapping iterations so that the mapper's own iteration count is not zero, and a ``Refiner`` on that map."""
    from test_gpu_mapping_mirror import _setup as mapping_setup
    from monogs_amd.refinement import Refiner
    frames, intr, gmap, mapper, bg = mapping_setup(3, 3)
    mapper.map_surgery = False
    mapper.optimize_map(frames, iters=MAPPER_ITERS)
    mapper._drop_plan()
    for vp in frames:                                   # (what the mapper's last backward left on the keyframes)
        for q in (vp.cam_rot_delta, vp.cam_trans_delta, vp.exposure_a, vp.exposure_b):
            q.grad = None
    gmap.optimizer.zero_grad(set_to_none=True)
    return frames, intr, gmap, bg, Refiner(gmap, intr, bg, seed=3, **kw)


def _snapshot(gmap):
    opt = gmap.optimizer
    return dict(params=[p.detach().cpu().clone() for p in gmap.params()], steps=opt.t_dev.cpu().clone(),
                lr=float(opt.device_lrs()[0]), max_radii=gmap.max_radii_2d.cpu().clone())


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


_EAGER = {}


def _eager_reference():
    """ONE eager run of 14 iterations, its state after 12 and after 14 (a sequence of 12 draws is a prefix of one of 14),
    shared by the tests that compare a captured run against it."""
    if not _EAGER:
        frames, intr, gmap, bg, refiner = _setup()
        before = [p.detach().cpu().clone() for p in gmap.params()]
        refiner.begin(frames, 14)
        for n in range(1, 15):
            refiner.step_eager()
            if n in (12, 14):
                _EAGER[n] = dict(_snapshot(gmap), before=before, sequence=list(refiner.sequence[:n]))
        assert refiner.stats["eager_iters"] == 14 and refiner.stats["replays"] == 0
        refiner.finish()
        refiner.close()
    return _EAGER


def _check_runs_agree(a, b, iters, tag):
    """The bars of ``_check_windows_agree`` (tests/test_gpu_window.py) that apply to a run without poses: equal step counts, the
    device-stepped xyz rate within 1e-7 relative, the update of the first four tensors within ``tol_update`` = 3e-2 relative L2
    (not the rotations: pure-noise gradients), ``max_radii_2d`` differing on < 1e-3 of the Gaussians."""
    assert torch.equal(a["steps"], b["steps"]) and int(a["steps"][0]) == MAPPER_ITERS + iters, (tag, a["steps"])
    assert abs(a["lr"] - b["lr"]) <= 1e-7 * b["lr"], (tag, a["lr"], b["lr"])
    worst = 0.0
    for x, y, s in list(zip(a["params"], b["params"], b["before"]))[:4]:
        assert (y - s).abs().max() > 0
        r = _rel(x - s, y - s)
        worst = max(worst, r)
        assert r < 3e-2, (tag, r)
    off = float((a["max_radii"] != b["max_radii"]).float().mean())
    assert off < 1e-3, (tag, off)
    print(f"{tag}: worst update relative L2 {worst:.3g} (bar 3e-2); max_radii_2d differs on {off:.3g} of the Gaussians (bar 1e-3); "
          f"xyz rate {a['lr']:.6g} vs {b['lr']:.6g}")


def test_refinement_iteration_matches_the_reference_loop_step_for_step(native_lib):
    """Six eager iterations, the mirror re-seeded from the driver before each (raw parameters, both moments, step counts; its xyz
    rate is its OWN ``expon_lr`` bookkeeping after the first).  Gradients: against the mirror's autograd through the torch loss.
    Optimiser: the driver's own gradients through ``torch.optim.Adam`` at the rate the mirror's schedule says applies, as part
    (c) of the mapping mirror test does (Adam normalises a gradient: noise-level entries would decide the comparison otherwise)."""
    from refinement_mirror import MirrorRefinement
    from test_gpu_mapping_mirror import CAP, _check_gradients, _check_optimizer, _poses
    from monogs_amd.gaussian_optim import expon_lr
    iters = 6
    frames, intr, gmap, bg, refiner = _setup()
    refiner.keep_grads = True
    mirror = MirrorRefinement(intr, bg, lambda_ssim=refiner.lambda_ssim, lr_schedule=gmap.lr_schedule)
    P, opt = len(gmap), gmap.optimizer
    assert P > 3000
    lr_mapper = expon_lr(MAPPER_ITERS, **gmap.lr_schedule)
    assert abs(opt.lrs[0] - lr_mapper) <= 1e-6 * lr_mapper and lr_mapper < 0.95 * gmap.lr_schedule["lr_init"]
    refiner.begin(frames, iters)
    assert len(refiner.sequence) == iters and len(set(refiner.sequence)) > 1            # more than one keyframe is drawn
    worst = dict(grad=0.0, off=0, loss=0.0)
    for n in range(1, iters + 1):
        lrs = [float(x) for x in opt.device_lrs().tolist()]
        if n > 1:
            lrs[0] = mirror.group("xyz")["lr"]
        mirror.load_map(gmap.params(), opt.exp_avg, opt.exp_avg_sq, opt.t_dev.tolist(), lrs, gmap.xyz_gradient_accum, gmap.denom,
                        gmap.max_radii_2d, gmap.kf_idx, gmap.nr_obs)
        mirror.load_keyframes(frames)
        accum, denom, poses, steps = gmap.xyz_gradient_accum.clone(), gmap.denom.clone(), _poses(frames), opt.t_dev.tolist()
        deltas = [(f.cam_rot_delta.detach().clone(), f.cam_trans_delta.detach().clone()) for f in frames]
        k = refiner.step_eager()
        assert k == refiner.sequence[n - 1]
        pkg, terms = mirror.forward_backward(k)
        # gradients of xyz / rgb / opacity / scaling: the "torch loss" bar of the mapping mirror test (relative L2 < 1e-3)
        worst["grad"] = max(worst["grad"], _check_gradients(refiner, mirror, (n, "torch loss"), "torch loss"))
        rg = refiner._buf.rg
        for name, got in (("loss", rg.loss), ("l1", rg.l1), ("ssim", rg.ssim)):
            # the value bar of tests/test_gpu_ssim.py (1e-4 absolute) on all three terms
            d = abs(float(got) - float(terms[name]))
            worst["loss"] = max(worst["loss"], d)
            assert d <= 1e-4, (n, name, float(got), float(terms[name]))
        mirror.statistics_and_step(pkg, gaussian_grads=refiner.last_grads)
        _check_optimizer(gmap, mirror, n)
        assert opt.t_dev.tolist() == [s + 1 for s in steps], (n, opt.t_dev.tolist())
        # max_radii_2d equal wherever the two renders' radii agree; the rest is capped
        agree = pkg["radii"] == refiner.last_radii
        off = int((~agree).sum())
        worst["off"] = max(worst["off"], off)
        assert off <= CAP * P, (n, off, P)
        assert torch.equal(gmap.max_radii_2d[agree], mirror.max_radii_2d[agree]) and float(mirror.max_radii_2d.max()) > 0, n
        # the densification statistics, the poses and the exposures are not the refinement's to touch
        assert torch.equal(gmap.xyz_gradient_accum, accum) and torch.equal(gmap.denom, denom), n
        for f, b, d in zip(frames, poses, deltas):
            assert torch.equal(f.R.cpu(), b[0]) and torch.equal(f.T.cpu(), b[1]), (n, f.frame_idx)
            assert torch.equal(f.exposure_a.data.cpu(), b[2]) and torch.equal(f.exposure_b.data.cpu(), b[3]), (n, f.frame_idx)
            assert torch.equal(f.cam_rot_delta.detach(), d[0]) and torch.equal(f.cam_trans_delta.detach(), d[1]), (n, f.frame_idx)
            assert all(q.grad is None for q in (f.cam_rot_delta, f.cam_trans_delta, f.exposure_a, f.exposure_b)), (n, f.frame_idx)
        # update_learning_rate(n) with the refinement's OWN count: expon_lr(n), not expon_lr(mapper iterations + n)
        lr, want, wrong = float(opt.device_lrs()[0]), expon_lr(n, **gmap.lr_schedule), expon_lr(MAPPER_ITERS + n, **gmap.lr_schedule)
        assert abs(lr - want) <= 1e-6 * want, (n, lr, want)           # the bar of test_captured_window_iteration_equals_eager
        assert abs(mirror.group("xyz")["lr"] - want) <= 1e-12 * want and abs(lr - wrong) > 1e-2 * want, (n, lr, wrong)
    out = refiner.finish()
    assert out["iters"] == iters and out["stats"]["eager_iters"] == iters and out["stats"]["captures"] == 0
    assert abs(opt.lrs[0] - expon_lr(iters, **gmap.lr_schedule)) <= 1e-6 * opt.lrs[0]         # synced back to the host copy
    refiner.close()
    print("worst / bar over %d iterations: gradients vs torch loss %.3g (bar 1e-3 relative L2); loss / L1 / SSIM values %.3g (bar "
          "1e-4); at most %d of %d Gaussians disagree on a radius (cap %d)" % (iters, worst["grad"], worst["loss"], worst["off"], P, int(CAP * P)))


def test_captured_refinement_matches_eager(native_lib):
    """Twelve iterations eager, twelve with ``use_graph=True``: one eager iteration, ONE capture, eleven replays."""
    iters = 12
    eager = _eager_reference()[iters]
    frames, intr, gmap, bg, refiner = _setup(use_graph=True)
    out = refiner.refine(frames, iters)
    assert refiner.sequence == eager["sequence"]
    assert out["stats"] == dict(captures=1, replays=iters - 1, eager_iters=1, overflow_redos=0), out["stats"]
    from monogs_amd import rasterizer
    assert not rasterizer.check_overflow()
    _check_runs_agree(_snapshot(gmap), eager, iters, "captured vs eager")
    assert all(p.grad is None for p in gmap.params())
    refiner.close()


def test_chunked_recapture_and_overflow_redo(native_lib):
    """14 iterations in chunks of at most 4 replays; the first capture reserves 0.3 of the measured instance count, so its chunk
    drops instances (the status-word path of tests/test_gpu_features.py::test_capacity_mode_matches_exact_path: a flag, not a
    fault), is rolled back and runs again from a capture with room."""
    from monogs_amd import rasterizer
    iters = 14
    eager = _eager_reference()[iters]
    frames, intr, gmap, bg, refiner = _setup(use_graph=True, max_replays_per_capture=4, first_reserve_scale=0.3)
    out = refiner.refine(frames, iters)
    st = out["stats"]
    print(f"chunked run: {st}")
    assert st["overflow_redos"] >= 1 and st["captures"] >= 3, st
    assert st["eager_iters"] == 1 and st["replays"] == iters - 1, st            # (replays that were rolled back do not count)
    assert st["captures"] == 4 + st["overflow_redos"], st                       # chunks of 4, 4, 4, 1
    assert refiner.sequence == eager["sequence"]
    _check_runs_agree(_snapshot(gmap), eager, iters, "chunked + redone vs eager")
    assert rasterizer.check_overflow() is False
    refiner.close()


def test_refinement_lowers_its_own_loss(native_lib):
    """80 captured iterations on the under-fitted map (one back-projected frame): the mean loss of the last quarter is strictly
    below that of the first quarter.  A sanity condition, no margin."""
    frames, intr, gmap, bg, refiner = _setup(use_graph=True)
    out = refiner.refine(frames, 80)
    print(f"first / last quarter means: {out['first']} / {out['last']}")
    assert out["window"] == 20 and out["stats"]["replays"] == 79
    for v in list(out["first"].values()) + list(out["last"].values()):
        assert v == v and abs(v) < 10.0
    assert out["last"]["loss"] < out["first"]["loss"], out
    # the terms are consistent: loss = (1 - lambda) L1 + lambda (1 - SSIM) holds for the means as well
    for part in (out["first"], out["last"]):
        assert abs(part["loss"] - (0.8 * part["l1"] + 0.2 * (1.0 - part["ssim"]))) <= 1e-5
    refiner.close()
