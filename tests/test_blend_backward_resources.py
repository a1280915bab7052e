"""blend_backward_s_kernel runs at eight waves per SIMD, unsplit and split (both walk directions compiled into one kernel).  The
compiler's resource report for gfx950 (no GPU needed) holds every instantiation -- <pose-only, split> x 2 x 2 -- to occupancy 8,
no scratch, at most 64 vector registers and at most 20 480 bytes of LDS per workgroup (eight workgroups in the compute unit's
160 KB)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")


def _resource_report(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the flags of blend.o in csrc/Makefile
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wno-unused-function", "-DNDEBUG",
           "-fno-slp-vectorize", "-Wno-inline-asm", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, "blend.hip"), "-o", str(tmp_path / "blend.o")]
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


def test_blend_backward_s_kernel_keeps_eight_waves_per_simd(tmp_path):
    kernels = _resource_report(tmp_path)
    bwd = {k: v for k, v in kernels.items() if "blend_backward_s_kernel" in k}
    assert len(bwd) == 4, sorted(kernels)
    for name, res in bwd.items():
        assert int(res["Occupancy [waves/SIMD]"]) == 8, (name, res)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, (name, res)
        assert int(res["LDS Size [bytes/block]"]) <= 20480, (name, res)
        assert int(res["VGPRs"]) <= 64, (name, res)
