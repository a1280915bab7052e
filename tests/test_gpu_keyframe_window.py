"""Device-side keyframe selection (csrc/kfwindow.hip, monogs_amd/keyframe_window.py) on the GPU (pytest -m gpu).

Every bar is exact equality -- the kernels count in integers -- except the three floats the decision reports, which are float32
evaluations of sums of at most ten products and are held to 1e-5 relative against the float64 mirror (tests/keyframe_mirror.py).
"""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest
import torch

import keyframe_mirror as km

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2049, 640 * 480)


def _same(got, ref):
    """value and count, with == (NaN where the mirror has NaN)."""
    (gv, gc), (rv, rc) = got, ref
    return gc == rc and ((math.isnan(gv) and math.isnan(rv)) or gv == rv)


def _gpu_median(v, mask=None, lo=0.0, scratch=None):
    from monogs_amd import keyframe_window as kw
    med, cnt = kw.masked_median(v.to(DEV), None if mask is None else mask.to(DEV), lo, scratch)
    return med.item(), cnt.item()


def _from_bits(bits):
    return bits.to(torch.int32).view(torch.float32)


def _distributions(n, g):
    """name -> (values, mask, lo)"""
    ri = lambda lo, hi: torch.randint(lo, hi, (n,), generator=g)  # noqa: E731
    holes = torch.rand(n, generator=g) < 0.2
    quant = ri(0, 8).float() / 8 + 0.5
    quant[holes] = 0.0
    low10 = _from_bits(0x40000000 + ri(0, 1024))
    signs = torch.randn(n, generator=g) * 3
    signs[holes] = 0.0
    signs[torch.rand(n, generator=g) < 0.1] = -0.0
    den = _from_bits(ri(0, 1 << 20) | (ri(0, 2) << 31))                  # +-denormals, +-0 among them
    den[holes] = -0.0
    tiny_mask = torch.where(torch.rand(n, generator=g) < 0.6, torch.tensor(1e-30), torch.tensor(0.0))
    return {
        "quantised": (quant, None, 0.0),
        "all_equal": (torch.full((n,), 2.5), None, 0.0),
        "low_10_bits": (low10, None, 0.0),
        "mixed_signs": (signs, None, -math.inf),
        "denormals": (den, None, 0.0),
        "denormals_all": (den, None, -math.inf),
        "tiny_mask": (quant, tiny_mask, 0.0),
    }


@pytest.mark.parametrize("n", SIZES)
def test_median_equals_torch_median_of_the_compacted_tensor(native_lib, n):
    from monogs_amd import keyframe_window as kw
    g = torch.Generator().manual_seed(100 + n)
    scratch = kw.median_scratch(n, DEV)
    for name, (v, mask, lo) in _distributions(n, g).items():
        scratch.fill_(0xFF)                                             # nothing is assumed about the scratch
        got, ref = _gpu_median(v, mask, lo, scratch), km.lower_median(v, mask, lo)
        print(f"n={n} {name}: kernel {got} mirror {ref}")
        assert _same(got, ref), (n, name, got, ref)
    # two calls back to back on one scratch, then nothing counted: NaN and 0
    d = _distributions(n, g)
    a = kw.masked_median(d["quantised"][0].to(DEV), None, 0.0, scratch)
    b = kw.masked_median(d["mixed_signs"][0].to(DEV), None, -math.inf, scratch)
    assert _same((a[0].item(), a[1].item()), km.lower_median(d["quantised"][0]))
    assert _same((b[0].item(), b[1].item()), km.lower_median(d["mixed_signs"][0], None, -math.inf))
    for v, mask, lo in ((torch.zeros(n), None, 0.0), (torch.ones(n), torch.zeros(n), 0.0), (torch.ones(n), None, math.inf)):
        med, cnt = _gpu_median(v, mask, lo, scratch)
        assert math.isnan(med) and cnt == 0


def test_median_of_nothing_and_the_reference_fixture(native_lib):
    from monogs_amd import keyframe_window as kw
    med, cnt = _gpu_median(torch.zeros(0))
    assert math.isnan(med) and cnt == 0
    gold = np.load(os.path.join(ROOT, "tests", "golden", "median_depth.npz"))
    depth, mask = torch.from_numpy(gold["depth"]), torch.from_numpy(gold["mask"])
    assert kw.median_depth(depth.to(DEV)).item() == float(gold["median_nomask"][0])
    assert kw.median_depth(depth.to(DEV), mask.to(DEV)).item() == float(gold["median_mask"][0])
    out = kw.median_depth(depth.to(DEV), mask.to(DEV).float())
    assert out.dim() == 0 and out.is_cuda and out.item() == float(gold["median_mask"][0])
    assert _gpu_median(depth, mask.float())[1] == int(gold["valid_mask"].sum())


def test_median_replays_from_a_captured_graph(native_lib):
    from monogs_amd import keyframe_window as kw
    n = 2049
    g = torch.Generator().manual_seed(9)
    v = torch.zeros(n, device=DEV)
    scratch = kw.median_scratch(n, DEV)
    med = torch.zeros((), device=DEV)
    cnt = torch.zeros((), dtype=torch.int32, device=DEV)
    kw._median_launch(v, None, 0.0, scratch, med, cnt)                 # (the code object is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kw._median_launch(v, None, 0.0, scratch, med, cnt)
    for rep in range(3):
        x = torch.rand(n, generator=g) * (rep + 1)
        x[torch.rand(n, generator=g) < 0.3] = 0.0
        v.copy_(x)
        scratch.fill_(0xFF if rep % 2 else 0)
        graph.replay()
        torch.cuda.synchronize()
        assert _same((med.item(), cnt.item()), km.lower_median(x)), rep


# ---- covisibility ------------------------------------------------------------------------------------------------------
def _covis(lib, P, K, rows, row_words, counts, cur_nt=None, cur_bits=None, cur_out=None):
    from monogs_amd import _lib
    kf_bits = (C.c_void_p * max(K, 1))(*[None if w == 0 else r.data_ptr() for r, w in zip(rows, row_words)])
    kf_words = (C.c_uint64 * max(K, 1))(*row_words)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.check(lib.mgs_covisibility(P, p(cur_nt), p(cur_bits), K, kf_bits, kf_words, p(cur_out), counts.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream), "mgs_covisibility")


@pytest.mark.parametrize("P", (1, 63, 64, 65, 4097))
@pytest.mark.parametrize("K", (1, 3, 32))
def test_covisibility_counts_equal_the_bool_tensor_counts(native_lib, P, K):
    from monogs_amd.gaussian_optim import window_stats
    from monogs_amd.keyframe_window import pack_visibility, unpack_visibility
    g = torch.Generator().manual_seed(1000 * P + K)
    words = (P + 63) // 64

    def touched():                      # negative, zero, small and extreme counts
        t = torch.randint(-3, 4, (P,), generator=g, dtype=torch.int32)
        t[torch.rand(P, generator=g) < 0.1] = 2 ** 31 - 1
        t[torch.rand(P, generator=g) < 0.1] = -2 ** 31
        return t
    nts = [touched() for _ in range(K)]
    cur = touched()
    dnts = [t.to(DEV) for t in nts]
    radii = [torch.ones(P, dtype=torch.int32, device=DEV) for _ in range(K)]
    f = lambda: torch.zeros(P, device=DEV)  # noqa: E731
    bits = torch.full((K, words), -1, dtype=torch.int64, device=DEV)
    window_stats([None] * K, radii, dnts, f(), f(), f(), False, bits)           # the rows come from mgs_window_stats itself
    rows = [bits[k] for k in range(K)]
    row_words = [words] * K
    ref_rows = [t > 0 for t in nts]
    row_words[0] = words - 1                                                    # one row shorter than the current one
    ref_rows[0] = ref_rows[0].clone()
    ref_rows[0][64 * (words - 1):] = False
    ref = km.overlap_counts(cur > 0, ref_rows)

    counts = torch.full((K, 4), -1, dtype=torch.int32, device=DEV)
    cur_out = torch.full((words,), -1, dtype=torch.int64, device=DEV)
    _covis(native_lib, P, K, rows, row_words, counts, cur_nt=cur.to(DEV), cur_out=cur_out)
    assert torch.equal(counts.cpu().long(), ref), (counts.cpu(), ref)
    assert torch.equal(unpack_visibility(cur_out.cpu(), P), cur > 0)
    assert not unpack_visibility(cur_out.cpu(), 64 * words)[P:].any()          # zero tail
    assert torch.equal(cur_out.cpu(), pack_visibility(cur > 0))

    # the packed form agrees, and bits at or beyond P never count (set in the current row and in the last keyframe's)
    dirty = torch.ones(64 * words, dtype=torch.bool)
    dirty[:P] = cur > 0
    dirty_row = torch.ones(64 * words, dtype=torch.bool)
    dirty_row[:P] = unpack_visibility(bits[K - 1].cpu(), P)
    rows2 = list(rows)
    if K > 1:
        rows2[K - 1] = pack_visibility(dirty_row).to(DEV)
    counts2 = torch.full((K, 4), -1, dtype=torch.int32, device=DEV)
    cur_out2 = torch.full((words,), -1, dtype=torch.int64, device=DEV)
    _covis(native_lib, P, K, rows2, row_words, counts2, cur_bits=pack_visibility(dirty).to(DEV), cur_out=cur_out2)
    assert torch.equal(counts2, counts) and torch.equal(cur_out2, cur_out)


# ---- the decision ------------------------------------------------------------------------------------------------------
def _close(got, ref):
    return (math.isnan(got) and math.isnan(ref)) or abs(got - ref) <= 1e-5 * abs(ref)


def test_decisions_match_the_mirror_on_the_seeded_windows(native_lib):
    """Every scenario through KeyframeWindow.observe: median, covisibility and decision kernels, one read-back, the list
    update.  The scenarios are well separated from every threshold (tests/test_keyframe_window_host.py), so the decisions are
    exact; the three floats are float32 against float64."""
    from monogs_amd.keyframe_window import KeyframeWindow, pack_visibility
    for sc in km.scenarios():
        prm = sc["prm"]
        K = prm["K"]
        ids = [100 - 3 * i for i in range(K)]                              # most recent first
        w = KeyframeWindow(prm["window_size"], check_viewpoints_overlap=bool(prm["check_overlap"]),
                           kf_interval=prm["kf_interval"], kf_cutoff=prm["kf_cutoff"])
        w.is_window_full = bool(prm["window_full"])
        w.cur_kf_list = list(ids)
        vp = [types.SimpleNamespace(R=R.to(DEV), T=T.to(DEV)) for R, T in sc["poses"]]
        w.viewpoints = dict(zip(ids, vp[1:]))
        for k, row in zip(ids, sc["rows"]):
            w.set_visibility(k, pack_visibility(row).to(DEV))
        frame = ids[0] + prm["frames_since_last_kf"]
        depth = torch.full((1, 6, 7), sc["median"], device=DEV)
        depth[0, 0, :3] = 0.0                                               # invalid pixels do not move the median
        pkg = dict(depth=depth, opacity=torch.ones(1, 6, 7, device=DEV), n_touched=sc["cur"].to(torch.int32).to(DEV))
        dec = w.observe(frame, vp[0], pkg)
        rec = w.last_record
        counts = km.overlap_counts(sc["cur"], sc["rows"])
        assert torch.equal(w.last_counts.cpu().long(), counts)
        median32 = float(torch.tensor(sc["median"], dtype=torch.float32))
        ref = km.decide(prm, counts, median32, sc["poses"], torch.float64)
        tag = (sc["seed"], sc["mode"], prm)
        print(f"seed {sc['seed']} K={K} {sc['mode']}: kernel {tuple(rec)} mirror {ref}")
        assert (rec.create_kf, rec.removed_by_cutoff, rec.removed_by_size) == \
            (ref["create_kf"], ref["removed_by_cutoff"], ref["removed_by_size"]), (tag, rec, ref)
        assert rec.median_depth == median32
        assert _close(rec.iou, ref["iou"]) and _close(rec.distance, ref["distance"]), (tag, rec, ref)
        new_list, removed = km.apply_to_list(ids, frame, ref)
        assert w.cur_kf_list == new_list and dec.removed_ids == removed and dec.create_kf == ref["create_kf"], tag
        if ref["create_kf"]:
            assert torch.equal(w.visibility[frame].cpu(), pack_visibility(sc["cur"]))
            assert set(w.visibility) == set(new_list) == set(w.viewpoints)


# ---- the harness -------------------------------------------------------------------------------------------------------
ROOM = dict(n_frames=10, intrinsics=dict(fx=535.4 / 4, fy=539.2 / 4, cx=320.1 / 4, cy=247.6 / 4, W=160, H=120),
            tracking_itr_num=10, mapping_itr_num=5, init_itr_num=20, window_size=4, kf_interval=1, scene="room")
PARENT_KEYS = {
    "kf_extend_s", "track_capture_s", "track_s", "track_iters", "tracked", "map_s", "map_iters", "keyframes", "renders", "surgery",
    "frames", "gaussians", "width", "height", "tracking_fps", "tracking_iters_per_s", "mapping_iters_per_s", "mapping_kf_per_s",
    "tracking_steady_iters_per_s", "mapping_steady_iters_per_s", "mapping_keyframe_iters_per_s", "mapping_replays",
    "mapping_eager_iters", "mapping_captures", "mapping_capture_s", "window_sizes", "kf_extend_ms", "ate_rmse_m",
    "track_iters_per_frame", "poses", "position_error_m", "camera_centers", "camera_centers_gt", "map_loss", "graph_tracking",
    "graph_mapping", "map_surgery", "config"}


@pytest.mark.parametrize("check", (False, True))
def test_harness_window_follows_the_mirror_frame_by_frame(native_lib, check):
    """run_slam(kf_selection="overlap") on the small room, teacher-forced: at every tracked frame the mirror decides from that
    frame's own n_touched, depth, poses and visibility rows (pulled to the CPU) and must arrive at the same window."""
    from monogs_amd.slam_harness import run_slam
    trace = []
    r = run_slam(kf_selection="overlap", check_viewpoints_overlap=check, kf_trace=trace, **ROOM)
    assert len(trace) == ROOM["n_frames"] - 1
    window = [0]
    n_kf = n_cut = n_size = 0
    for t in trace:
        assert t["window_before"] == window
        cur = t["n_touched"] > 0
        counts = km.overlap_counts(cur, [t["visibility"][k] for k in window])
        median, _ = km.lower_median(t["depth"], t["opacity"])
        prm = dict(km.DEFAULTS, K=len(window), window_size=ROOM["window_size"], window_full=int(t["is_window_full"]),
                   check_overlap=int(check), kf_interval=ROOM["kf_interval"], frames_since_last_kf=t["frame"] - window[0])
        ref = km.decide(prm, counts, median, [t["poses"][k] for k in [t["frame"]] + window], torch.float64)
        rec = t["record"]
        print(f"frame {t['frame']}: window {window} kernel {tuple(rec)} mirror {ref}")
        assert rec.median_depth == median
        assert (rec.create_kf, rec.removed_by_cutoff, rec.removed_by_size) == \
            (ref["create_kf"], ref["removed_by_cutoff"], ref["removed_by_size"]), (t["frame"], rec, ref)
        window, removed = km.apply_to_list(window, t["frame"], ref)
        assert t["window_after"] == window and t["decision"].removed_ids == removed
        n_kf += ref["create_kf"]
        n_cut += ref["create_kf"] and ref["removed_by_cutoff"] >= 0
        n_size += ref["create_kf"] and ref["removed_by_size"] >= 0
    assert (r["keyframes_selected"], r["evicted_by_cutoff"], r["evicted_by_size"]) == (n_kf, n_cut, n_size)
    assert r["final_window"] == window and r["keyframes"] == n_kf + 1 and len(window) <= ROOM["window_size"]
    if not check:                       # the fork's setting: every frame a keyframe, the window overflows and evicts
        assert n_kf == ROOM["n_frames"] - 1 and n_cut + n_size >= ROOM["n_frames"] - ROOM["window_size"]


def test_interval_selection_returns_exactly_the_parent_keys(native_lib):
    from monogs_amd.slam_harness import run_slam
    r = run_slam(**dict(ROOM, n_frames=3, kf_interval=2))
    assert set(r) == PARENT_KEYS
    with pytest.raises(ValueError, match="kf_selection"):
        run_slam(kf_selection="covisibility", **ROOM)
