"""The stereo kernels (csrc/stereo.hip): the compiler's resource report for gfx950 (no GPU needed) must show no scratch and no
LDS for every one of them and full occupancy (8 waves per SIMD, i.e. at most 64 VGPRs) for the streaming kernels.  The path
kernels are bound by their dependent chain, not by occupancy: their registers are printed (and recorded in DESIGN.md), and
held only to what the design needs -- one wave per SIMD is what a frame gives them anyway."""
from resource_report import resource_report

STREAMING = ("stereo_prepare_kernel", "stereo_prefilter_kernel", "stereo_hsum_kernel", "stereo_vsum_kernel",
             "stereo_winner_kernel", "stereo_table_kernel", "stereo_finish_kernel")


def test_stereo_kernels(tmp_path):
    report, stderr = resource_report("stereo.hip", tmp_path)
    assert "warning:" not in stderr, stderr[-4000:]
    kernels = {k: v for k, v in report.items() if "stereo_" in k}
    count = lambda s: sum(s in k for k in kernels)      # noqa: E731
    # prepare <REMAP>, path <DIR, ADD> for the five directions, one of everything else
    assert count("stereo_prepare_kernel") == 2 and count("stereo_path_kernel") == 5, sorted(kernels)
    assert len(kernels) == 2 + 5 + 6, sorted(kernels)
    for name, res in sorted(kernels.items()):
        what = (name, "VGPRs", res["VGPRs"], "occupancy", res["Occupancy [waves/SIMD]"], "LDS bytes", res["LDS Size [bytes/block]"], res)
        print(what[:7])
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
        assert int(res["LDS Size [bytes/block]"]) == 0, what
        if any(s in name for s in STREAMING):
            assert int(res["Occupancy [waves/SIMD]"]) == 8 and int(res["VGPRs"]) <= 64, what
        else:
            assert "stereo_path_kernel" in name, name
            # two blocks of ST_UNROLL cost words and sum words in flight, plus addressing: well inside half the file
            assert int(res["VGPRs"]) <= 128, what
