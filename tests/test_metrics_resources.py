"""The image-metrics kernels (csrc/metrics.hip) are streaming kernels bound by memory: the compiler's resource report for
gfx950 (no GPU needed) must show no scratch, full occupancy (8 waves per SIMD, i.e. at most 64 VGPRs) and no LDS beyond the
48 bytes of the workgroup sum (four doubles + four counts)."""
from resource_report import resource_report


def test_metrics_kernels_stream(tmp_path):
    report, stderr = resource_report("metrics.hip", tmp_path)
    assert "warning:" not in stderr, stderr[-4000:]
    kernels = report
    main = {k: v for k, v in kernels.items() if "metrics_kernel" in k}
    fin = {k: v for k, v in kernels.items() if "metrics_finalize_kernel" in k}
    assert len(main) == 2 and len(fin) == 1, sorted(kernels)        # <VEC = true>, <VEC = false>
    for name, res in {**main, **fin}.items():
        what = (name, "VGPRs", res["VGPRs"], "LDS bytes", res["LDS Size [bytes/block]"], res)
        print(what[:5])
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
        assert int(res["Occupancy [waves/SIMD]"]) == 8 and int(res["VGPRs"]) <= 64, what       # built: 52 (vector), 26 (scalar), 20
        assert int(res["LDS Size [bytes/block]"]) <= 48, what                                  # built: 48
