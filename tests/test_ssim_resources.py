"""The SSIM kernels are streaming kernels: the compiler's resource report for gfx950 (no GPU needed) must show no scratch, at
least 4 waves per SIMD and at most 40 960 bytes of LDS per 256-thread workgroup (four workgroups per compute unit) -- the
floors -- and what csrc/ssim.hip actually reaches: forward 5 waves and 26 912 bytes (six workgroups by LDS), backward
6 waves and 21 672 bytes (seven)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")


def _resource_report(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the flags of ssim.o in csrc/Makefile
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
           "-DNDEBUG", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, "ssim.hip"), "-o", str(tmp_path / "ssim.o")]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[-Rpass-analysis", line)
        if m and name:
            kernels[name][m.group(1).strip()] = m.group(2)
    return kernels


def test_makefile_builds_ssim_with_the_flags_used_here():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bssim\.hip\b", mk, flags=re.M)
    assert "-O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -fno-gpu-rdc -Wall -Wno-unused-function -DNDEBUG" in mk
    assert not re.search(r"ssim\.o:\s*CXXFLAGS", mk)          # no per-file flags to mirror


def test_ssim_kernels_stream(tmp_path):
    kernels = _resource_report(tmp_path)
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
