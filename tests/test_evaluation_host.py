"""Host side of the evaluation and of the refinement driver (no GPU): ``eval_ate`` against closed forms, the frame selection of
``eval_rendering``, the keyframe order of ``Refiner`` and the argument errors of ``mgs_image_metrics``.

``evo`` is not installed where this suite runs, so ``align=True`` is held against transforms whose answer
is known in closed form; parity with evo's own ``align`` is unpinned."""
import math
import random
import types

import numpy as np
import pytest
import torch


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def _path(n=17, seed=3):
    """Ground-truth camera-to-world poses along a curve that spans all three axes."""
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 1.0, n)
    c = np.stack([1.5 * np.sin(2.2 * s), 0.4 * s ** 2 - 0.1, 2.0 * s + 0.3 * np.cos(5 * s)], 1) + 0.01 * rng.standard_normal((n, 3))
    Rs = [_rot(rng.standard_normal(3), 0.4 * rng.standard_normal()) for _ in range(n)]
    return Rs, c


def _frames(Rs_gt, c_gt, Rs_est, c_est):
    """Frames as the harness keeps them: world-to-camera ``R``, ``T`` (estimate) and ``R_gt``, ``T_gt`` in float64 tensors."""
    out = []
    for i, (Rg, cg, Re, ce) in enumerate(zip(Rs_gt, c_gt, Rs_est, c_est)):
        w2c = lambda R, c: (torch.tensor(R.T), torch.tensor(-R.T @ c))  # noqa: E731
        Rw, Tw = w2c(Re, ce)
        Rgw, Tgw = w2c(Rg, cg)
        out.append(types.SimpleNamespace(frame_idx=i, R=Rw, T=Tw, R_gt=Rgw, T_gt=Tgw))
    return out


def _moved(Rs, c, A, t, s=1.0):
    """The trajectory with every camera centre x replaced by (A^-1 (x - t)) / s, so that s A x' + t = x brings it back."""
    Ai = np.linalg.inv(A)
    return [Ai @ R for R in Rs], (c - t) @ Ai.T / s


def test_ate_of_a_rigidly_moved_path_is_zero_after_alignment_and_closed_form_without():
    from monogs_amd.evaluation import eval_ate
    Rs, c = _path()
    A, t = _rot([0.3, -1.0, 0.5], 0.7), np.array([0.4, -1.1, 2.5])
    Re, ce = _moved(Rs, c, A, t)
    frames = _frames(Rs, c, Re, ce)
    got = eval_ate(frames, align=True)
    print(f"rigid: aligned rmse {got['rmse']:.3g} (bar 1e-9)")
    assert got["rmse"] <= 1e-9 and got["max"] <= 1e-9 and got["n"] == len(frames)
    e = np.linalg.norm(c - ce, axis=1)
    plain = eval_ate(frames)
    assert abs(plain["rmse"] - math.sqrt(float(np.mean(e ** 2)))) <= 1e-12 * plain["rmse"] and plain["rmse"] > 0.5
    for k, v in (("mean", e.mean()), ("median", np.median(e)), ("min", e.min()), ("max", e.max())):
        assert abs(plain[k] - float(v)) <= 1e-12 * abs(float(v)), k
    assert plain["aligned"] is False and got["aligned"] is True
    # align=False is what the reference reports: correct_scale changes nothing there
    assert eval_ate(frames, correct_scale=True)["rmse"] == plain["rmse"]


def test_ate_of_a_similarity_needs_correct_scale():
    from monogs_amd.evaluation import eval_ate
    Rs, c = _path(seed=5)
    A, t, s = _rot([1.0, 0.2, 0.1], -1.1), np.array([-2.0, 0.3, 0.9]), 1.37
    Re, ce = _moved(Rs, c, A, t, s)
    frames = _frames(Rs, c, Re, ce)
    sim = eval_ate(frames, align=True, correct_scale=True)
    print(f"similarity: aligned rmse {sim['rmse']:.3g} (bar 1e-9)")
    assert sim["rmse"] <= 1e-9
    rigid = eval_ate(frames, align=True)                     # a rigid fit cannot undo the scale
    assert rigid["rmse"] > 1e-2
    e = np.linalg.norm(c - ce, axis=1)
    assert abs(eval_ate(frames)["rmse"] - math.sqrt(float(np.mean(e ** 2)))) <= 1e-12 * eval_ate(frames)["rmse"]


def test_umeyama_takes_the_reflection_branch_and_still_returns_a_rotation():
    """A mirrored copy: the unconstrained least-squares fit is a reflection (det < 0), the answer must be the best ROTATION."""
    from monogs_amd.evaluation import eval_ate, umeyama
    Rs, c = _path(seed=9)
    M = np.diag([1.0, 1.0, -1.0])
    ce = c @ M.T
    cov = (c - c.mean(0)).T @ (ce - ce.mean(0))
    U, _, Vt = np.linalg.svd(cov)
    assert np.linalg.det(U) * np.linalg.det(Vt) < 0                 # the branch is taken
    R, t, s = umeyama(ce, c, with_scale=False)
    assert abs(np.linalg.det(R) - 1.0) <= 1e-12 and np.allclose(R @ R.T, np.eye(3), atol=1e-12) and s == 1.0
    # optimal among rotations: no other rotation near it does better, and the reflection itself would give zero
    res = lambda Rm: float(np.sum(((ce - ce.mean(0)) @ Rm.T - (c - c.mean(0))) ** 2))  # noqa: E731
    best = res(R)
    rng = np.random.default_rng(0)
    for _ in range(200):
        assert res(_rot(rng.standard_normal(3), 0.05 * rng.standard_normal()) @ R) >= best - 1e-9
    assert res(M) <= 1e-20 < best
    frames = _frames(Rs, c, [M @ Rm for Rm in Rs], ce)
    got = eval_ate(frames, align=True)
    assert abs(got["rmse"] - math.sqrt(best / len(c))) <= 1e-9


def test_ate_over_a_keyframe_subset_and_a_single_pose():
    from monogs_amd.evaluation import eval_ate
    Rs, c = _path()
    rng = np.random.default_rng(1)
    ce = c + 0.05 * rng.standard_normal(c.shape)
    frames = _frames(Rs, c, Rs, ce)
    ids = [0, 4, 5, 11, 16]
    e = np.linalg.norm(c[ids] - ce[ids], axis=1)
    got = eval_ate(frames, kf_ids=ids)
    assert got["n"] == 5 and abs(got["rmse"] - math.sqrt(float(np.mean(e ** 2)))) <= 1e-12
    assert abs(got["median"] - float(np.median(e))) <= 1e-12
    one = eval_ate(frames, kf_ids=[7])
    assert one["n"] == 1 and abs(one["rmse"] - float(np.linalg.norm(c[7] - ce[7]))) <= 1e-12
    assert one["rmse"] == one["mean"] == one["median"] == one["min"] == one["max"]
    assert eval_ate(frames, kf_ids=[7], align=True, correct_scale=True)["rmse"] <= 1e-12        # one point aligns onto its target
    assert eval_ate(frames, kf_ids=[])["n"] == 0


@pytest.mark.parametrize("n", [1, 2, 6, 11, 12])
def test_frames_evaluated(n):
    from monogs_amd.evaluation import eval_frame_indices
    want = {1: [], 2: [0], 6: [0], 11: [0, 5], 12: [0, 5, 10]}[n]          # range(0, n - 1, 5)
    assert eval_frame_indices(n, []) == want
    assert eval_frame_indices(n, [0, 5, 10]) == []                          # keyframes at the multiples of 5: nothing left
    assert eval_frame_indices(n, [0, 3, 4]) == [i for i in want if i != 0]
    assert eval_frame_indices(n, [5]) == [i for i in want if i != 5]
    assert eval_frame_indices(n, [1, 2], interval=1) == [i for i in range(n - 1) if i not in (1, 2)]


def test_refiner_sequence_is_a_fresh_random_stream():
    from monogs_amd.refinement import Refiner
    for seed, K, iters in ((0, 7, 500), (5, 1, 20), (11, 30, 26000)):
        rng = random.Random(seed)
        assert Refiner.draw_sequence(K, iters, seed) == [rng.randint(0, K - 1) for _ in range(iters)]
    a, b = Refiner.draw_sequence(7, 500, 0), Refiner.draw_sequence(7, 500, 1)
    assert a != b and a == Refiner.draw_sequence(7, 500, 0)
    assert set(a) == set(range(7))


def test_image_metrics_argument_errors(native_lib):
    """NULL pointers and empty sizes come back as 1 with a message, before anything is launched (no device needed)."""
    lib = native_lib
    ok = 0x1000                                          # non-NULL, never dereferenced
    good = [16, 16, ok, ok, ok, None, ok, ok, None]      # (u8_out and the stream may be NULL)
    for k in (2, 3, 4, 6, 7):
        args = list(good)
        args[k] = None
        assert lib.mgs_image_metrics(*args) == 1, k
        assert b"non-NULL" in lib.mgs_last_error(), (k, lib.mgs_last_error())
    for w, h in ((0, 16), (16, 0), (-1, 16), (0, 0)):
        assert lib.mgs_image_metrics(w, h, *good[2:]) == 1, (w, h)
        assert b"positive" in lib.mgs_last_error()
    assert lib.mgs_image_metrics(40000, 40000, *good[2:]) == 1 and b"2^31" in lib.mgs_last_error()
    a, b = lib.mgs_metrics_scratch_bytes(640, 480), lib.mgs_metrics_scratch_bytes(1200, 680)
    assert 16 <= a <= b and a % 16 == 0 and lib.mgs_metrics_scratch_bytes(0, 0) >= 16
    assert lib.mgs_metrics_scratch_bytes(640, 480) == a                     # pure
