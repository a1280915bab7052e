"""The blend forward runs at eight waves per SIMD; the per-tile depth sort folded into it (blend_forward_kernel<true>) must
not cost a wave.  The compiler's resource report for gfx950 (no GPU needed) holds every instantiation to occupancy 8,
no scratch and at most 20 480 bytes of LDS per workgroup (eight workgroups in the compute unit's 160 KB)."""
from resource_report import resource_report


def test_blend_forward_keeps_eight_waves_per_simd(tmp_path):
    kernels = resource_report("blend.hip", tmp_path)[0]
    fwd = {k: v for k, v in kernels.items() if "blend_forward_kernel" in k}
    assert len(fwd) == 2, sorted(kernels)                 # <false>: depth-ordered lists, <true>: sorts its tile first
    for name, res in fwd.items():
        assert int(res["Occupancy [waves/SIMD]"]) == 8, (name, res)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, (name, res)
        assert int(res["LDS Size [bytes/block]"]) <= 20480, (name, res)
        assert int(res["VGPRs"]) <= 64 and int(res["TotalSGPRs"]) <= 80, (name, res)
