"""The frame-ingest kernels (csrc/ingest.hip) are streaming kernels and a 3x3 stencil, bound by memory: the compiler's resource
report for gfx950 (no GPU needed) must show no scratch, full occupancy (8 waves per SIMD, i.e. at most 64 VGPRs) and no LDS for
every one of them, on the vector and on the scalar route."""
from resource_report import resource_report


def test_ingest_kernels_stream(tmp_path):
    report, stderr = resource_report("ingest.hip", tmp_path)
    assert "warning:" not in stderr, stderr[-4000:]
    kernels = {k: v for k, v in report.items() if "ingest_" in k}
    count = lambda s: sum(s in k for k in kernels)      # noqa: E731
    # prepare <VEC, REMAP>, intensity <VEC>, threshold <VEC>
    assert (count("ingest_prepare_kernel"), count("ingest_intensity_kernel"), count("ingest_threshold_kernel")) == (4, 2, 2), sorted(kernels)
    assert len(kernels) == 8, sorted(kernels)
    for name, res in kernels.items():
        what = (name, "VGPRs", res["VGPRs"], "LDS bytes", res["LDS Size [bytes/block]"], res)
        print(what[:5])
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
        # built: prepare 47 / 59 / 18 / 38, intensity 62 (vector) / 46, threshold 10 / 4
        assert int(res["Occupancy [waves/SIMD]"]) == 8 and int(res["VGPRs"]) <= 64, what
        assert int(res["LDS Size [bytes/block]"]) == 0, what
