"""The mesh-rendering kernels (csrc/mesh_render.hip) and the Depth L1 pair (csrc/metrics.hip): the compiler's
resource report for gfx950 (no GPU needed) must show each of them exactly once, no scratch, no compiler warning and an occupancy of
at least 4 waves per SIMD.  The register, occupancy and LDS figures are printed; DESIGN.md ("Mesh rendering") quotes them."""
from resource_report import resource_report

KERNELS = {
    "mesh_render.hip": ("mesh_render_clear_kernel", "mesh_render_setup_kernel", "mesh_render_scan_local_kernel",
                        "mesh_render_scan_blocks_kernel", "mesh_render_raster_kernel", "mesh_render_resolve_kernel"),
    "metrics.hip": ("depth_l1_partial_kernel", "depth_l1_finish_kernel"),
}


def test_mesh_render_kernels_do_not_spill(tmp_path):
    for unit, kernels in KERNELS.items():
        report, stderr = resource_report(unit, tmp_path)
        assert "warning:" not in stderr, stderr[-4000:]
        for want in kernels:
            found = {k: v for k, v in report.items() if want in k}
            assert len(found) == 1, (want, sorted(report))
            (name, res), = found.items()
            what = (name, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "waves/SIMD", res["Occupancy [waves/SIMD]"],
                    "LDS bytes", res["LDS Size [bytes/block]"])
            print(what)
            assert int(res["ScratchSize [bytes/lane]"]) == 0, what
            assert int(res["Occupancy [waves/SIMD]"]) >= 4, what
