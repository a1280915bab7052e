"""The result dict of ``run_slam`` as a contract: which keys it holds in which flag combination, which of them are None, the
values the schedule fixes, and the accuracy -- against a recording made once, on the MI355X, at the commit BEFORE the harness
was split into modules (``tests/golden/run_slam_contract.json``; ``python tests/test_gpu_slam_contract.py --record`` wrote it).

The configuration is the smallest this project has measured to track: the room of tests/test_gpu_object_layer.py (160x120, 12
frames, 600 initialisation / 60 mapping / <= 100 tracking iterations, window 4, every second frame a keyframe; 0.8 s a run).
Two runs of one sequence are not bit-identical (the order of the blend backward's float atomics differs), so the accuracy bar is
the one tests/test_gpu_slam.py derives for two runs of one sequence: ATE and worst frame at most twice the recorded run's +
1.5 mm (15 % of the ~1 cm the camera moves per frame).  The recorded figures are in the JSON."""
import json
import os
import sys

import pytest
import torch  # noqa: F401  (before the native library is loaded, as in every other GPU test module)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_slam_contract.json")
ROOM = dict(n_frames=12, intrinsics=dict(fx=535.4 / 4, fy=539.2 / 4, cx=320.1 / 4, cy=247.6 / 4, W=160, H=120),
            tracking_itr_num=100, mapping_itr_num=60, init_itr_num=600, window_size=4, kf_interval=2, scene="room")
RUNS = dict(
    eager={},
    graph_overlap=dict(graph_tracking=True, graph_mapping=True, kf_selection="overlap"),
    eval_refine=dict(eval_render=True, refine_iters=5),
    objects=dict(nr_objects=18),               # ROOM_SURFACES: six walls + three face axes of each of the four boxes
)
SCHEDULE_KEYS = ("frames", "tracked", "keyframes", "map_iters", "window_sizes", "config", "width", "height",
                 "graph_tracking", "graph_mapping", "map_surgery")
RENDERS_FIXED = ("eager", "eval_refine", "objects")      # eager mapping: renders - track_iters = map_iters x window, no re-runs


def key_shape(d, prefix=""):
    """{dotted key path: whether its value is None}, through every nested dict with string keys."""
    out = {}
    for k, v in d.items():
        out[prefix + k] = v is None
        if isinstance(v, dict) and all(isinstance(x, str) for x in v):
            out.update(key_shape(v, prefix + k + "."))
    return out


def summarize(name, r):
    schedule = {k: r[k] for k in SCHEDULE_KEYS}
    sizes = r["surgery"]["gaussians_after_keyframe"]
    schedule["gaussians_after_keyframe_len"], schedule["gaussians_after_first_keyframe"] = len(sizes), sizes[0]
    if name in RENDERS_FIXED:
        schedule["renders_minus_track_iters"] = r["renders"] - r["track_iters"]
    return dict(keys=key_shape(r), schedule=schedule, ate_rmse_m=r["ate_rmse_m"], worst_position_error_m=max(r["position_error_m"]))


def run(name):
    from monogs_amd.slam_harness import run_slam
    return json.loads(json.dumps(summarize(name, run_slam(**RUNS[name], **ROOM))))      # (as the recording reads back: lists, no tuples)


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module", params=list(RUNS))
def pair(request, native_lib, recorded):
    return request.param, run(request.param), recorded[request.param]


def test_result_keys_and_nones(pair):
    name, now, rec = pair
    assert now["keys"] == rec["keys"], (name, sorted(set(now["keys"].items()) ^ set(rec["keys"].items())))


def test_schedule_values(pair):
    name, now, rec = pair
    assert now["schedule"] == rec["schedule"], (name, now["schedule"], rec["schedule"])


def test_accuracy(pair):
    name, now, rec = pair
    print(f"{name}: ATE {now['ate_rmse_m'] * 1e3:.2f} mm (recorded {rec['ate_rmse_m'] * 1e3:.2f}), worst frame "
          f"{now['worst_position_error_m'] * 1e3:.2f} mm (recorded {rec['worst_position_error_m'] * 1e3:.2f})")
    assert now["ate_rmse_m"] <= 2 * rec["ate_rmse_m"] + 1.5e-3
    assert now["worst_position_error_m"] <= 2 * rec["worst_position_error_m"] + 1.5e-3


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        raise SystemExit("usage: python tests/test_gpu_slam_contract.py --record [FILE]")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = sys.argv[2] if len(sys.argv) == 3 else GOLDEN
    with open(out, "w") as f:
        json.dump({name: run(name) for name in RUNS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)
