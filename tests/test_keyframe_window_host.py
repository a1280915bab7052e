"""Keyframe selection and window management without a GPU: the C ABI's argument errors (nothing is launched), the scratch size,
`KeyframeWindow`'s list handling driven by hand-made decision records, the packed-row helpers, and the decision scenarios of
tests/test_gpu_keyframe_window.py: well separated from every threshold, and decided alike by the float32 and the float64
mirror (tests/keyframe_mirror.py)."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import keyframe_mirror as km

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mgs_median_scratch_bytes", "mgs_masked_median", "mgs_covisibility", "mgs_keyframe_decide")
PTR = 0x1000                          # non-NULL and never dereferenced


def _err(lib):
    return lib.mgs_last_error().decode()


def test_header_declares_the_entry_points(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES and hasattr(native_lib, s)
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 14
    assert "raises" in text[text.index("mgs_masked_median:"):text.index("mgs_covisibility:")]      # the c == 0 difference is stated
    assert C.sizeof(_lib.MgsKeyframeParams) == 11 * 4


def test_median_scratch_is_pure_and_monotone(native_lib):
    f = native_lib.mgs_median_scratch_bytes
    sizes = [f(n) for n in (0, 1, 63, 4096, 4097, 640 * 480, 1200 * 680, 1 << 24, (1 << 32) - 1)]
    assert sizes == sorted(sizes) and sizes[0] >= 64 and sizes[-1] <= 1 << 20
    assert f(640 * 480) == f(640 * 480) == sizes[5]


def test_median_refuses_bad_arguments_before_any_launch(native_lib):
    m = native_lib.mgs_masked_median
    assert m(PTR, None, 1 << 32, 0.0, PTR, PTR, PTR, None) == 1 and "2^32" in _err(native_lib)
    assert m(PTR, None, 16, 0.0, None, PTR, PTR, None) == 1 and "non-NULL" in _err(native_lib)
    assert m(PTR, None, 16, 0.0, PTR, None, PTR, None) == 1 and "non-NULL" in _err(native_lib)
    assert m(PTR, None, 16, 0.0, PTR, PTR, None, None) == 1 and "non-NULL" in _err(native_lib)
    assert m(None, None, 16, 0.0, PTR, PTR, PTR, None) == 1 and "values" in _err(native_lib)
    assert m(PTR, None, 16, float("nan"), PTR, PTR, PTR, None) == 1 and "NaN" in _err(native_lib)


def test_covisibility_refuses_bad_arguments_before_any_launch(native_lib):
    cv = native_lib.mgs_covisibility
    rows = (C.c_void_p * 33)(*[PTR] * 33)
    words = (C.c_uint64 * 33)(*[2] * 33)
    assert cv(100, PTR, None, 33, rows, words, None, PTR, None) == 1 and "0..32" in _err(native_lib)
    assert cv(-1, PTR, None, 2, rows, words, None, PTR, None) == 1
    assert cv(100, PTR, PTR, 2, rows, words, None, PTR, None) == 1 and "exactly one" in _err(native_lib)
    assert cv(100, None, None, 2, rows, words, None, PTR, None) == 1 and "exactly one" in _err(native_lib)
    assert cv(100, PTR, None, 2, rows, words, None, None, None) == 1 and "non-NULL" in _err(native_lib)
    assert cv(100, PTR, None, 2, None, words, None, PTR, None) == 1 and "non-NULL" in _err(native_lib)
    rows[1] = None
    assert cv(100, PTR, None, 2, rows, words, None, PTR, None) == 1 and "NULL keyframe row" in _err(native_lib)
    # nothing to count: returns 0 without a launch (this machine has no device)
    assert cv(100, PTR, None, 0, None, None, None, None, None) == 0
    assert cv(0, PTR, None, 2, rows, words, None, PTR, None) == 1          # (the NULL row is still refused)
    rows[1] = PTR
    assert cv(0, PTR, None, 2, rows, words, None, PTR, None) == 0


def test_decide_refuses_bad_arguments_before_any_launch(native_lib):
    from monogs_amd import _lib
    kd = native_lib.mgs_keyframe_decide
    poses = (C.c_void_p * 68)(*[PTR] * 68)
    good = dict(K=3, window_size=8, window_full=0, check_overlap=1, kf_interval=1, frames_since_last_kf=1, kf_translation=0.08,
                kf_min_translation=0.05, kf_overlap=0.9, kf_cutoff=0.4, n_dont_touch=2)
    prm = _lib.MgsKeyframeParams(**good)
    assert kd(None, PTR, PTR, poses, PTR, None) == 1 and "non-NULL" in _err(native_lib)
    assert kd(C.byref(prm), None, PTR, poses, PTR, None) == 1 and "non-NULL" in _err(native_lib)
    assert kd(C.byref(prm), PTR, None, poses, PTR, None) == 1 and "non-NULL" in _err(native_lib)
    assert kd(C.byref(prm), PTR, PTR, None, PTR, None) == 1 and "non-NULL" in _err(native_lib)
    assert kd(C.byref(prm), PTR, PTR, poses, None, None) == 1 and "non-NULL" in _err(native_lib)
    for bad, msg in ((dict(K=33), "1..32"), (dict(K=0), "1..32"), (dict(window_size=0), "at least 1"),
                     (dict(n_dont_touch=0), "at least 1")):
        p = _lib.MgsKeyframeParams(**dict(good, **bad))
        assert kd(C.byref(p), PTR, PTR, poses, PTR, None) == 1 and msg in _err(native_lib), bad
    poses[5] = None                                                        # T of the second window keyframe
    assert kd(C.byref(prm), PTR, PTR, poses, PTR, None) == 1 and "NULL pose" in _err(native_lib)


def test_python_entry_points_have_no_cpu_path(native_lib):
    from monogs_amd import keyframe_window as kw
    with pytest.raises(RuntimeError, match="no CPU path"):
        kw.median_depth(torch.rand(1, 8, 8))
    w = kw.KeyframeWindow(8)
    w.bootstrap(0, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        w.launch(1, None, torch.rand(1, 8, 8), None, torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match="bootstrap"):
        kw.KeyframeWindow(8).launch(1, None, torch.rand(1, 8, 8), None, torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match="window_size"):
        kw.KeyframeWindow(33)


def test_window_list_handling_follows_add_to_window():
    from monogs_amd.keyframe_window import DecisionRecord, KeyframeWindow
    w = KeyframeWindow(4, latch_window_full=True)
    w.bootstrap(0, "vp0")
    assert w.cur_kf_list == [0] and not w.is_window_full
    assert w.apply_decision(1, DecisionRecord(False, 2, -1)) == [] and w.cur_kf_list == [0]     # not a keyframe: nothing moves
    for i in (1, 2, 3):
        assert w.apply_decision(i, DecisionRecord(True, -1, -1), f"vp{i}", torch.tensor([i])) == []
    assert w.cur_kf_list == [3, 2, 1, 0] and w.is_window_full                                    # front insertion, latched
    assert w.viewpoints[2] == "vp2" and int(w.visibility[3][0]) == 3
    # the size eviction alone: position 3 of [4, 3, 2, 1, 0]
    assert w.apply_decision(4, DecisionRecord(True, -1, 3), "vp4", torch.tensor([4])) == [1]
    assert w.cur_kf_list == [4, 3, 2, 0] and 1 not in w.viewpoints and 1 not in w.visibility
    # both removals in one call, cut-off first: positions 4 and 2 of [5, 4, 3, 2, 0]
    assert w.apply_decision(5, DecisionRecord(True, 4, 2), "vp5", torch.tensor([5])) == [0, 3]
    assert w.cur_kf_list == [5, 4, 2] and w.is_window_full
    # the two protected slots (the new frame and the last keyframe) cannot leave; nor can a slot beyond the list
    for pos in (0, 1, 4):
        with pytest.raises(ValueError, match="protected or missing"):
            w.apply_decision(6, DecisionRecord(True, pos, -1), "vp6")
    assert w.cur_kf_list == [5, 4, 2]
    prm = w.params(7)
    assert (prm.K, prm.window_size, prm.window_full, prm.frames_since_last_kf, prm.n_dont_touch) == (3, 4, 1, 2, 2)
    assert abs(prm.kf_translation - 0.08) < 1e-7 and abs(prm.kf_min_translation - 0.05) < 1e-7
    assert abs(prm.kf_overlap - 0.9) < 1e-7 and prm.check_overlap == 0 and prm.kf_interval == 1        # the fork's defaults
    fork = KeyframeWindow(2)
    fork.bootstrap(0)
    fork.apply_decision(1, DecisionRecord(True, -1, -1))
    assert not fork.is_window_full                                          # the fork never sets the flag


def test_packed_rows_and_prune():
    from monogs_amd.keyframe_window import KeyframeWindow, pack_visibility, unpack_visibility
    g = torch.Generator().manual_seed(5)
    for P in (1, 63, 64, 65, 200):
        m = torch.rand(P, generator=g) < 0.5
        words = pack_visibility(m)
        assert words.dtype == torch.int64 and words.numel() == (P + 63) // 64
        assert torch.equal(unpack_visibility(words, P), m)
        assert torch.equal(pack_visibility(m.to(torch.int32) * 7), words)                  # n_touched packs as > 0
        assert not unpack_visibility(words, P + 130)[P:].any()                             # a short row is zero-extended
        for i in range(P):                                                                 # bit i of word w = element 64 w + i
            assert bool((int(words[i // 64]) >> (i % 64)) & 1) == bool(m[i])
    P = 150
    a, b, keep = (torch.rand(P, generator=g) < 0.5 for _ in range(3))
    w = KeyframeWindow(8)
    w.bootstrap(0, None, a)
    w.set_visibility(3, pack_visibility(b))
    w.prune(keep)
    n = int(keep.sum())
    assert torch.equal(unpack_visibility(w.visibility[0], n), a[keep]) and torch.equal(unpack_visibility(w.visibility[3], n), b[keep])
    with pytest.raises(ValueError, match="packed words"):
        w.set_visibility(1, torch.zeros(4, dtype=torch.float32))


def test_mirror_median_is_the_lower_median():
    v = torch.tensor([3.0, -1.0, 0.0, 2.0, 5.0, 4.0])
    assert km.lower_median(v) == (3.0, 4)                                    # of 2 3 4 5: rank (4 - 1) // 2
    assert km.lower_median(v, torch.tensor([1.0, 1.0, 1.0, 0.0, 1e-30, 1.0])) == (4.0, 3)
    assert km.lower_median(v, lo=-math.inf) == (2.0, 6)
    med, c = km.lower_median(v, lo=10.0)
    assert math.isnan(med) and c == 0


def test_scenarios_are_well_separated_and_precision_independent():
    """The condition on the inputs of the GPU decision test: every ratio at least 1e-4 from its threshold, the two best scores
    at least 1e-3 (relative) apart -- and then float32 and float64 decide alike."""
    scs = km.scenarios()
    assert 38 <= len(scs) <= 48
    seen = dict(both=0, none=0, cutoff_only=0, size_only=0, several=0, protected=0, empty=0, refused=0, created=0)
    for sc in scs:
        counts = km.overlap_counts(sc["cur"], sc["rows"])
        d64 = km.decide(sc["prm"], counts, sc["median"], sc["poses"], torch.float64)
        d32 = km.decide(sc["prm"], counts, sc["median"], sc["poses"], torch.float32)
        assert d64["margin"] >= 1e-4 and d64["score_gap"] >= 1e-3, (sc["seed"], d64)
        for k in ("create_kf", "removed_by_cutoff", "removed_by_size"):
            assert d32[k] == d64[k], (sc["seed"], k, d32, d64)
        cut, size = d64["removed_by_cutoff"], d64["removed_by_size"]
        assert cut == -1 or 2 <= cut <= sc["prm"]["K"]
        assert size == -1 or (2 <= size <= sc["prm"]["K"] and size != cut)
        seen["both"] += cut >= 0 and size >= 0
        seen["none"] += cut < 0 and size < 0
        seen["cutoff_only"] += cut >= 0 and size < 0
        seen["size_only"] += cut < 0 and size >= 0
        seen["protected"] += sc["prm"]["K"] <= 2
        seen["empty"] += sc["mode"] == "empty"
        seen["created"] += d64["create_kf"]
        seen["refused"] += not d64["create_kf"]
        if sc["mode"] == "several" and sc["prm"]["K"] >= 4:
            cutoff = sc["prm"]["kf_cutoff"] if sc["prm"]["window_full"] else 0.4
            low = [i for i in range(2, sc["prm"]["K"] + 1)
                   if float(counts[i - 1, 0]) / float(min(counts[i - 1, 2], counts[i - 1, 3])) <= cutoff]
            assert len(low) >= 2 and cut == max(low)                        # several candidates: the last goes
            seen["several"] += 1
        if sc["mode"] == "empty":                                           # 0/0 everywhere: NaN creates and removes nothing
            assert math.isnan(d64["iou"]) and cut == -1
            if sc["prm"]["check_overlap"] and sc["prm"]["K"] < sc["prm"]["window_size"]:
                assert not d64["create_kf"]
    assert all(v > 0 for v in seen.values()), seen
    assert {sc["prm"]["K"] for sc in scs} == set(range(1, 12)) and {sc["prm"]["window_size"] for sc in scs} == {8, 10}
    assert {sc["prm"]["window_full"] for sc in scs} == {0, 1} and {sc["prm"]["check_overlap"] for sc in scs} == {0, 1}
