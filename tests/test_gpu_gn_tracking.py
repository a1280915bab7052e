"""The Gauss-Newton tracker (monogs_amd/gn_tracking.py) on the GPU, with the Adam ``TrackingGraph`` as the yardstick: the set-up of
tests/test_gpu_slam.py::test_graph_tracking_equals_eager_tracking at a quarter of the fr3_office size (160 x 120) -- a 3-frame
sequence of 30 000 Gaussians, a map of 80 initialisation iterations, frozen, each frame started from the previous true pose."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K160 = dict(fx=535.4 / 4, fy=539.2 / 4, cx=320.1 / 4, cy=247.6 / 4, W=160, H=120)
RUN = dict(n_frames=5, intrinsics=K160, tracking_itr_num=100, mapping_itr_num=30, window_size=8, kf_interval=2, init_itr_num=80,
           n_gaussians=30000)


@pytest.fixture(scope="module")
def world(native_lib):
    from monogs_amd.gaussian_map import GaussianMap
    from monogs_amd.mapping import WindowMapper
    from monogs_amd.sequences import make_sequence
    frames, intr = make_sequence(3, K160, n_gaussians=30000, device=DEV)
    bg = torch.zeros(3, device=DEV)
    gmap = GaussianMap(DEV)
    frames[0].update_RT(frames[0].R_gt.clone(), frames[0].T_gt.clone())
    gmap.extend_from_frame(frames[0], intr, downsample=8, init=True, point_size=1.0)
    mapper = WindowMapper(gmap, intr, bg, window_size=8)
    mapper.map_surgery = False
    mapper.optimize_map([frames[0]], iters=80, init=True)
    for p in gmap.params():
        p.grad = None
    return frames, intr, gmap, bg


def _start(frames, i, monocular=False):
    from monogs_amd.frames import Viewpoint
    f = frames[i]
    vp = Viewpoint(f.frame_idx, f.rgb, None if monocular else f.depth, DEV, gt_R=f.R_gt, gt_T=f.T_gt,
                   sensor="monocular" if monocular else "depth")
    vp.update_RT(frames[i - 1].R_gt.clone(), frames[i - 1].T_gt.clone())
    return vp


def _centre_error(vp):
    from monogs_amd.frames import position_error
    return position_error(vp).item()


def test_gauss_newton_tracks_in_fewer_iterations_than_adam(world):
    from monogs_amd.gn_tracking import GaussNewtonGraph, track_gauss_newton
    from monogs_amd.tracking import TrackingGraph
    frames, intr, gmap, bg = world
    for i in (1, 2):
        va = _start(frames, i)
        tg = TrackingGraph(va, intr, gmap, bg)
        n_adam = tg.track(va, 100)
        tg.close()
        e_adam = _centre_error(va)
        # ---- eager Gauss-Newton
        ve = _start(frames, i)
        e_start = _centre_error(ve)
        n_eager = track_gauss_newton(ve, intr, gmap, bg, 100)
        e_eager = _centre_error(ve)
        # ---- captured Gauss-Newton
        vg = _start(frames, i)
        gg = GaussNewtonGraph(vg, intr, gmap, bg)
        n_graph = gg.track(vg, 100)
        flag_up, steps, status = float(gg.opt.out[0]) > 0.5, int(gg.steps.item()), float(gg.opt.out[3])
        gg.close()
        e_graph = _centre_error(vg)
        print(f"frame {i}: start {e_start:.3e} m; Adam {n_adam} iterations -> {e_adam:.3e} m; Gauss-Newton eager {n_eager} -> {e_eager:.3e} m, "
              f"captured {n_graph} -> {e_graph:.3e} m")
        assert 1 < n_adam < 100
        assert n_eager < 100 and flag_up and status == 0                     # converged: the flag is up
        assert steps == n_graph, (steps, n_graph)                            # a surplus replay after convergence is a no-op
        assert e_eager <= max(2 * e_adam, 1e-4) and e_graph <= max(2 * e_adam, 1e-4), (e_eager, e_graph, e_adam)
        assert n_eager < n_adam and n_graph < n_adam, (n_eager, n_graph, n_adam)
        assert (ve.R - vg.R).abs().max() < 1e-5 and (ve.T - vg.T).abs().max() < 1e-5
        info = vg.gn_information
        assert info.shape == (6, 6) and info.dtype == torch.float64 and torch.linalg.eigvalsh(info.cpu()).min().item() > 0


def test_a_monocular_viewpoint_runs(world):
    from monogs_amd.gn_tracking import GaussNewtonGraph, track_gauss_newton
    frames, intr, gmap, bg = world
    ve = _start(frames, 1, monocular=True)
    e0 = _centre_error(ve)
    n_eager = track_gauss_newton(ve, intr, gmap, bg, 100)
    vg = _start(frames, 1, monocular=True)
    gg = GaussNewtonGraph(vg, intr, gmap, bg)
    n_graph = gg.track(vg, 100)
    gg.close()
    print(f"monocular: {n_eager} / {n_graph} iterations, centre error {e0:.3e} -> {_centre_error(ve):.3e} / {_centre_error(vg):.3e} m")
    assert n_eager < 100 and n_graph < 100
    assert _centre_error(ve) < e0 and _centre_error(vg) < e0
    with pytest.raises(ValueError, match="captured for a"):
        gg2 = GaussNewtonGraph(_start(frames, 1), intr, gmap, bg)
        try:
            gg2.track(_start(frames, 2, monocular=True), 5)
        finally:
            gg2.close()


def test_run_slam_with_the_gauss_newton_tracker(native_lib):
    from monogs_amd.slam_harness import run_slam
    gn = run_slam(tracker="gauss_newton", graph_tracking=True, **RUN)
    adam = run_slam(tracker="adam", **RUN)
    plain = run_slam(**RUN)
    print(f"run_slam: Gauss-Newton ATE {gn['ate_rmse_m']:.3e} m, iterations per frame {gn['track_iters_per_frame']}; "
          f"Adam ATE {adam['ate_rmse_m']:.3e} m, iterations per frame {adam['track_iters_per_frame']}")
    assert gn["tracker"] == "gauss_newton" and gn["ate_rmse_m"] < 2e-3, gn["ate_rmse_m"]
    assert set(adam) == set(plain) and "tracker" not in plain and set(gn) == set(plain) | {"tracker"}
    assert adam["ate_rmse_m"] < 2e-3 and plain["ate_rmse_m"] < 2e-3
    assert adam["config"] == plain["config"] and adam["frames"] == plain["frames"] and adam["tracked"] == plain["tracked"]
    with pytest.raises(ValueError, match="tracker"):
        run_slam(tracker="newton", **RUN)
