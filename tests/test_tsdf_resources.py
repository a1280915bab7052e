"""The TSDF kernels (csrc/tsdf.hip) are one lane per voxel with a handful of live values; the emit kernels unroll seven edges and six
tetrahedra.  The compiler's resource report for gfx950 (no GPU needed) must show no scratch for any kernel of the file.  The register,
occupancy and LDS figures are printed; DESIGN.md ("TSDF fusion and mesh extraction") quotes them."""
from resource_report import resource_report

KERNELS = ("tsdf_integrate_kernel", "tsdf_classify_kernel", "tsdf_cells_kernel", "tsdf_edges_kernel", "tsdf_scan_local_kernel",
           "tsdf_scan_blocks_kernel", "tsdf_emit_vertices_kernel", "tsdf_emit_triangles_kernel")


def test_tsdf_kernels_do_not_spill(tmp_path):
    report, stderr = resource_report("tsdf.hip", tmp_path)
    assert "warning:" not in stderr, stderr[-4000:]
    kernels = {k: v for k, v in report.items() if "tsdf_" in k}
    for want in KERNELS:
        assert sum(1 for k in kernels if want in k) == 1, (want, sorted(kernels))
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for name, res in kernels.items():
        what = (name, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "waves/SIMD", res["Occupancy [waves/SIMD]"],
                "LDS bytes", res["LDS Size [bytes/block]"])
        print(what)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
        assert int(res["Occupancy [waves/SIMD]"]) >= 4, what           # one-lane-per-voxel streaming: latency is hidden by waves
    # the only LDS is the scans' per-wave totals: 4 words, and 16 double words
    lds = {k: int(v["LDS Size [bytes/block]"]) for k, v in kernels.items()}
    assert all(b == 0 for k, b in lds.items() if "scan" not in k), lds
    assert all(b <= 128 for b in lds.values()), lds
