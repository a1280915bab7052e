"""Host side of the object layer's loss and score (monogs_amd/object_layer.py, the ``mgs_label_*`` entry points, the PLY rows):
what can be checked without a GPU -- versions, argument errors raised before anything is launched, the scores of a hand-made
confusion matrix, the PLY round trip."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P1 = 0x1000          # non-NULL and never dereferenced: every argument check comes before the first launch


def test_versions_agree(native_lib):
    from monogs_amd import _lib
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    assert int(re.search(r"#define MGS_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 21
    assert native_lib.mgs_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define MGS_LABEL_SCRATCH_LOSS (\d+)", text).group(1)) == 0
    assert native_lib.mgs_label_scratch_bytes() >= 16 + 8 and native_lib.mgs_label_scratch_bytes() % 8 == 0
    for name in ("mgs_label_scratch_bytes", "mgs_label_prepare", "mgs_label_loss_grads", "mgs_label_confusion"):
        assert name in _lib.SIGNATURES


def _calls(lib):
    """name -> f(W, H, K, pointers...) with the pointer arguments in declaration order."""
    return {
        "mgs_label_prepare": (lambda W, H, K, *p: lib.mgs_label_prepare(W, H, K, *p, None), ("labels", "valid", "scratch", "count_out")),
        "mgs_label_loss_grads": (lambda W, H, K, *p: lib.mgs_label_loss_grads(W, H, K, *p, None),
                                 ("feat", "labels", "valid", "count", "scratch", "d_feat")),
        "mgs_label_confusion": (lambda W, H, K, *p: lib.mgs_label_confusion(W, H, K, *p, None),
                                ("pred", "gt", "valid", "counts", "side")),
    }


def test_bad_arguments_return_1_before_any_launch(native_lib):
    for name, (call, ptrs) in _calls(native_lib).items():
        ok = [None if p == "valid" else P1 for p in ptrs]           # valid may be NULL; everything else is required
        for W, H, K, needle in ((8, 8, 0, b"K must be"), (8, 8, 257, b"K must be"), (8, 8, -1, b"K must be"),
                                (0, 8, 4, b"size must be positive"), (8, 0, 4, b"size must be positive"),
                                (-3, 8, 4, b"size must be positive"), (1 << 16, 1 << 15, 4, b"2^31")):
            assert call(W, H, K, *ok) == 1, (name, W, H, K)
            msg = native_lib.mgs_last_error()
            assert needle in msg and name.encode() in msg, (name, msg)
        for i, p in enumerate(ptrs):
            if p == "valid":
                continue
            args = list(ok)
            args[i] = None
            assert call(8, 8, 4, *args) == 1, (name, p)
            assert b"non-NULL" in native_lib.mgs_last_error() and p.encode() in native_lib.mgs_last_error(), (name, p)
    # a scratch that cannot hold the 8-byte partials
    for name in ("mgs_label_prepare", "mgs_label_loss_grads"):
        call, ptrs = _calls(native_lib)[name]
        args = [None if p == "valid" else (P1 + 4 if p == "scratch" else P1) for p in ptrs]
        assert call(8, 8, 4, *args) == 1 and b"8-byte aligned" in native_lib.mgs_last_error(), name


def test_cpu_tensors_and_wide_ids_are_refused_in_python(monkeypatch):
    from monogs_amd import _lib, object_layer as ol

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(ValueError, match="0..255"):
        ol.LabelTarget(torch.tensor([[0, 3], [256, 1]]))
    with pytest.raises(ValueError, match="0..255"):
        ol.LabelTarget(torch.tensor([[0, -1]], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ol.LabelTarget(torch.zeros(4, 5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ol.LabelTarget(torch.zeros(4, 5, dtype=torch.long))
    with pytest.raises(TypeError, match="integer"):
        ol.LabelTarget(torch.zeros(4, 5))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ol.label_loss_grads(torch.zeros(3, 4, 5), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ol.get_loss_labels(torch.zeros(3, 4, 5, requires_grad=True), None)
    with pytest.raises(ValueError, match="1..256"):
        ol._check_k(257)
    with pytest.raises(ValueError, match="learn_objects needs nr_objects"):
        from monogs_amd.gaussian_map import GaussianMap
        GaussianMap("cpu", learn_objects=True)
    import monogs_amd
    assert monogs_amd.ObjectLayerTrainer is ol.ObjectLayerTrainer and monogs_amd.segmentation_scores is ol.segmentation_scores


def test_segmentation_scores_on_a_hand_made_matrix():
    from monogs_amd.object_layer import segmentation_scores
    #            pred 0  1  2  3
    c = np.array([[5, 1, 0, 0],        # gt 0: 6 pixels
                  [2, 3, 0, 0],        # gt 1: 5 pixels
                  [0, 0, 0, 0],        # gt 2: absent from the ground truth AND from the prediction: left out of the mean
                  [0, 4, 0, 0]])       # gt 3: never predicted: IoU 0, but it occurs
    s = segmentation_scores(c)
    assert s["pixel_accuracy"] == pytest.approx(8 / 15)
    assert s["iou"][0] == pytest.approx(5 / 8) and s["iou"][1] == pytest.approx(3 / 10) and s["iou"][3] == 0.0
    assert np.isnan(s["iou"][2]) and s["classes"] == 3
    assert s["miou"] == pytest.approx((5 / 8 + 3 / 10 + 0.0) / 3)
    # the same from a device-style int32 tensor, counts above 2^31 read as unsigned
    big = torch.tensor([[-2 ** 31, 0], [0, 2 ** 31 - 1]], dtype=torch.int32)
    assert segmentation_scores(big)["pixel_accuracy"] == 1.0 and segmentation_scores(big)["miou"] == 1.0
    empty = segmentation_scores(np.zeros((3, 3)))
    assert np.isnan(empty["pixel_accuracy"]) and np.isnan(empty["miou"]) and empty["classes"] == 0
    with pytest.raises(ValueError, match="square"):
        segmentation_scores(np.zeros((2, 3)))


def _map_tensors(P=37, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(P, w, generator=g) for w in (3, 3, 1, 1, 4)]


def test_ply_round_trip_with_and_without_rows(tmp_path):
    from monogs_amd.ply_io import attribute_names, load_ply, read_vertex_table, save_ply
    ts = _map_tensors()
    rows = torch.randn(37, 18, generator=torch.Generator().manual_seed(1))
    rows[3, 5] = 1e-40                                            # a subnormal and a negative zero travel bit for bit
    rows[4, 0] = -0.0
    with_rows, plain, positional = (str(tmp_path / n) for n in ("rows.ply", "plain.ply", "positional.ply"))
    save_ply(with_rows, *ts, obj_prob=rows)
    save_ply(plain, *ts, obj_prob=None)
    save_ply(positional, *ts)
    m = load_ply(with_rows)
    assert set(m) == {"xyz", "f_dc", "opacity", "scaling", "rotation", "obj_prob"}
    assert m["obj_prob"].dtype == torch.float32 and m["obj_prob"].shape == (37, 18)
    assert np.array_equal(m["obj_prob"].numpy().view(np.uint32), rows.numpy().view(np.uint32))
    for k, t in zip(("xyz", "f_dc", "opacity", "scaling", "rotation"), ts):
        assert torch.equal(m[k], t), k
    names = list(read_vertex_table(with_rows))
    assert names == attribute_names(3, 1, 4, 18) and names[-19] == "rot_3" and names[-18:] == [f"obj_prob_{i}" for i in range(18)]
    # without the rows: the file save_ply has always written, byte for byte -- header and table stated here independently
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 37\n"
              + "".join(f"property float {n}\n" for n in ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity",
                                                            "scale_0", "rot_0", "rot_1", "rot_2", "rot_3"]) + "end_header\n")
    table = np.concatenate([ts[0].numpy(), np.zeros((37, 3), np.float32)] + [t.numpy() for t in ts[1:]], axis=1).astype("<f4")
    expected = header.encode("ascii") + table.tobytes()
    assert open(plain, "rb").read() == expected == open(positional, "rb").read()
    assert set(load_ply(plain)) == {"xyz", "f_dc", "opacity", "scaling", "rotation"}
    with pytest.raises(ValueError, match="rows"):
        save_ply(str(tmp_path / "bad.ply"), *ts, obj_prob=rows[:5])
