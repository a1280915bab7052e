"""blend_backward_s_kernel runs at eight waves per SIMD, unsplit and split (both walk directions compiled into one kernel).  The
compiler's resource report for gfx950 (no GPU needed) holds every instantiation -- <pose-only, split> x 2 x 2 -- to occupancy 8,
no scratch, at most 64 vector registers and at most 20 480 bytes of LDS per workgroup (eight workgroups in the compute unit's
160 KB)."""
from resource_report import resource_report


def test_blend_backward_s_kernel_keeps_eight_waves_per_simd(tmp_path):
    kernels = resource_report("blend.hip", tmp_path)[0]
    bwd = {k: v for k, v in kernels.items() if "blend_backward_s_kernel" in k}
    assert len(bwd) == 4, sorted(kernels)
    for name, res in bwd.items():
        assert int(res["Occupancy [waves/SIMD]"]) == 8, (name, res)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, (name, res)
        assert int(res["LDS Size [bytes/block]"]) <= 20480, (name, res)
        assert int(res["VGPRs"]) <= 64, (name, res)
