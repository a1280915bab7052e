"""The diagnostic kernel behind mgs_debug_blend_mask_stats (the forward's survivor masks against the backward's own cull) is not
on the hot path; the compiler's resource report for gfx950 (no GPU needed) holds it to "no scratch".  The hot kernels it sits
beside are held by test_blend_forward_resources.py and test_blend_backward_resources.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")


def test_mask_stats_kernel_has_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the flags of blend.o in csrc/Makefile
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wno-unused-function", "-DNDEBUG",
           "-fno-slp-vectorize", "-Wno-inline-asm", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, "blend.hip"), "-o", str(tmp_path / "blend.o")]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    scratch, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    mine = {k: v for k, v in scratch.items() if "blend_mask_stats_kernel" in k}
    assert len(mine) == 1, sorted(scratch)
    assert list(mine.values()) == [0], mine
