"""The kernels of csrc/mesheval.hip: the compiler's resource report for gfx950 (no GPU needed) must show every kernel of the file
exactly once and no scratch for any of them.  The register, occupancy and LDS figures are printed; DESIGN.md ("Reconstruction
evaluation") quotes them."""
from resource_report import resource_report

KERNELS = ("nn_all_pairs_kernel", "nn_query_kernel", "nn_empty_kernel", "mesh_area_kernel", "mesh_scan_local_kernel",
           "mesh_scan_blocks_kernel", "mesh_sample_kernel", "mesh_mark_seen_kernel", "recon_partial_kernel", "recon_finish_kernel")


def test_mesheval_kernels_do_not_spill(tmp_path):
    report, stderr = resource_report("mesheval.hip", tmp_path)
    assert "warning:" not in stderr, stderr[-4000:]
    kernels = {k: v for k, v in report.items() if "zero_fill" not in k}          # (common.h's clears are instantiated in every unit)
    for want in KERNELS:
        assert sum(1 for k in kernels if want in k) == 1, (want, sorted(kernels))
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for name, res in kernels.items():
        what = (name, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "waves/SIMD", res["Occupancy [waves/SIMD]"],
                "LDS bytes", res["LDS Size [bytes/block]"])
        print(what)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
        assert int(res["Occupancy [waves/SIMD]"]) >= 4, what
    lds = {k: int(v["LDS Size [bytes/block]"]) for k, v in kernels.items()}
    # the all-pairs tile (1024 float4), one staged box per wave (4 x 64 float4), the scans' and sums' per-wave totals
    assert max(b for k, b in lds.items() if "nn_all_pairs" in k) == 16384 and max(b for k, b in lds.items() if "nn_query" in k) == 4096
    assert all(b <= 512 for k, b in lds.items() if "nn_all_pairs" not in k and "nn_query" not in k), lds
