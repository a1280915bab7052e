"""The keyframe-window kernels in the compiler's resource report for gfx950 (no GPU needed): none of them spills to
private-memory scratch -- the covisibility and the decision kernel index pointer tables in their kernel arguments by lane, which
must stay loads from the argument segment -- and the LDS of the median's kernels is what csrc/kfwindow.hip says: one histogram of
2048 buckets (8192 bytes) per workgroup of the counting launch, the summed histogram plus 256 scan words (9216 bytes) in the
selecting launch."""
from resource_report import resource_report


def test_kfwindow_kernels_use_no_scratch_and_the_recorded_lds(tmp_path):
    kernels = resource_report("kfwindow.hip", tmp_path)[0]
    pick = lambda s: {k: v for k, v in kernels.items() if s in k}  # noqa: E731
    hist, select = pick("median_hist_kernel"), pick("median_select_kernel")
    covis, decide = pick("covisibility_kernel"), pick("keyframe_decide_kernel")
    assert len(hist) == 3 and len(select) == 3 and len(covis) == 1 and len(decide) == 1, sorted(kernels)     # <PASS> 0, 1, 2
    for name, res in {**hist, **select, **covis, **decide}.items():
        assert int(res["ScratchSize [bytes/lane]"]) == 0, (name, res)
        assert int(res["Occupancy [waves/SIMD]"]) >= 4, (name, res)
    for name, res in hist.items():
        assert int(res["LDS Size [bytes/block]"]) == 2048 * 4, (name, res)
    for name, res in select.items():
        assert int(res["LDS Size [bytes/block]"]) == (2048 + 256) * 4, (name, res)
    for name, res in {**covis, **decide}.items():
        assert int(res["LDS Size [bytes/block]"]) <= 2048, (name, res)
