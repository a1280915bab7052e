"""The feature kernels (csrc/features.hip) keep a chunk of C accumulators (forward) or C upstream gradients (backward) per lane.
The compiler's resource report for gfx950 (no GPU needed) must show no scratch for any instantiation: a spilled chunk is a
wrong choice of C, not something to accept.  The register, occupancy and LDS figures are printed; DESIGN.md section 3 quotes
the ones that were built."""
from resource_report import resource_report


def test_feature_kernels_do_not_spill(tmp_path):
    report, stderr = resource_report("features.hip", tmp_path)
    assert "warning:" not in stderr, stderr[-4000:]
    kernels = report
    fwd = {k: v for k, v in kernels.items() if "features_forward_kernel" in k}
    bwd = {k: v for k, v in kernels.items() if "features_backward_kernel" in k}
    empty = {k: v for k, v in kernels.items() if "features_empty_kernel" in k}
    assert len(fwd) == 3 and len(bwd) == 3 and len(empty) == 1, sorted(kernels)        # C = 4, 8, 16 each way
    for name, res in {**fwd, **bwd, **empty}.items():
        what = (name, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "waves/SIMD", res["Occupancy [waves/SIMD]"],
                "LDS bytes", res["LDS Size [bytes/block]"])
        print(what)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
    # built (VGPRs / waves per SIMD): forward C = 4: 23 / 8, C = 8: 31 / 8, C = 16: 47 / 8; backward 24 / 8, 32 / 8, 48 / 8;
    # no LDS anywhere.  (C = 32, not built: 80 and 74 VGPRs, 6 waves, the forward at 106 SGPRs.)
