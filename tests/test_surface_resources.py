"""The surface kernels (csrc/surface.hip) in the compiler's resource report for gfx950 (no GPU needed): neither the walk (three
instantiations: median with the early leave, median + variance, variance) nor the normals kernel spills to scratch, the walk uses no
LDS, and the unit compiles without a warning.  Registers, SGPRs and occupancy are printed; DESIGN.md section 3 ("Surface depth")
quotes them."""
from resource_report import resource_report


def test_surface_kernels_do_not_spill_and_the_walk_uses_no_lds(tmp_path):
    report, stderr = resource_report("surface.hip", tmp_path)
    assert "warning:" not in stderr, stderr[-4000:]
    walks = {k: v for k, v in report.items() if "surface_depth_kernel" in k}
    normals = {k: v for k, v in report.items() if "depth_normals_kernel" in k}
    assert len(walks) == 3 and len(normals) == 1, sorted(report)
    for name, res in {**walks, **normals}.items():
        what = (name, "VGPRs", res["VGPRs"], "AGPRs", res.get("AGPRs"), "SGPRs", res["TotalSGPRs"], "waves/SIMD",
                res["Occupancy [waves/SIMD]"], "LDS bytes", res["LDS Size [bytes/block]"])
        print(what)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
    for name, res in walks.items():
        assert int(res["LDS Size [bytes/block]"]) == 0, (name, res)
        assert int(res["Occupancy [waves/SIMD]"]) == 8, (name, res)          # about eight values per lane: the SIMD stays full
