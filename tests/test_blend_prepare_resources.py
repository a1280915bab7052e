"""The diagnostic kernel behind mgs_debug_blend_mask_stats (the forward's survivor masks against the backward's own cull, in
csrc/blend_stats.hip) is not on the hot path; the compiler's resource report for gfx950 (no GPU needed) holds it to "no scratch".
The hot kernels are held by test_blend_forward_resources.py and test_blend_backward_resources.py."""
from resource_report import resource_report


def test_mask_stats_kernel_has_no_scratch(tmp_path):
    kernels = resource_report("blend_stats.hip", tmp_path)[0]
    scratch = {k: int(v["ScratchSize [bytes/lane]"]) for k, v in kernels.items()}
    mine = {k: v for k, v in scratch.items() if "blend_mask_stats_kernel" in k}
    assert len(mine) == 1, sorted(scratch)
    assert list(mine.values()) == [0], mine
