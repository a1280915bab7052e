"""The SSIM kernels are streaming kernels: the compiler's resource report for gfx950 (no GPU needed) must show no scratch, at
least 4 waves per SIMD and at most 40 960 bytes of LDS per 256-thread workgroup (four workgroups per compute unit) -- the
floors -- and what csrc/ssim.hip actually reaches: forward 5 waves and 26 912 bytes (six workgroups by LDS), backward
6 waves and 21 672 bytes (seven)."""
from resource_report import resource_report


def test_ssim_kernels_stream(tmp_path):
    kernels = resource_report("ssim.hip", tmp_path)[0]
    fwd = {k: v for k, v in kernels.items() if "ssim_forward_kernel" in k}
    bwd = {k: v for k, v in kernels.items() if "ssim_backward_kernel" in k}
    fin = {k: v for k, v in kernels.items() if "ssim_finalize_kernel" in k}
    assert len(fwd) == 2 and len(bwd) == 2 and len(fin) == 1, sorted(kernels)     # <TRAIN>, <REFINE>
    for name, res in {**fwd, **bwd, **fin}.items():
        assert int(res["ScratchSize [bytes/lane]"]) == 0, (name, res)
        assert int(res["Occupancy [waves/SIMD]"]) >= 4, (name, res)
        assert int(res["LDS Size [bytes/block]"]) <= 40960, (name, res)
    for name, res in fwd.items():
        assert int(res["Occupancy [waves/SIMD]"]) >= 5 and int(res["VGPRs"]) <= 96, (name, res)
        assert int(res["LDS Size [bytes/block]"]) <= 26912, (name, res)
    for name, res in bwd.items():
        assert int(res["Occupancy [waves/SIMD]"]) >= 6 and int(res["VGPRs"]) <= 80, (name, res)
        assert int(res["LDS Size [bytes/block]"]) <= 21672, (name, res)
