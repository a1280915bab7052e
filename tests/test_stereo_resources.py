"""The stereo kernels (csrc/stereo.hip): the compiler's resource report for gfx950 (no GPU needed) must show no scratch and no
LDS for every one of them and full occupancy (8 waves per SIMD, i.e. at most 64 VGPRs) for the streaming kernels.  The path
kernels are bound by their dependent chain, not by occupancy: their registers are printed (and recorded in DESIGN.md), and
held only to what the design needs -- one wave per SIMD is what a frame gives them anyway."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")
STREAMING = ("stereo_prepare_kernel", "stereo_prefilter_kernel", "stereo_hsum_kernel", "stereo_vsum_kernel",
             "stereo_winner_kernel", "stereo_table_kernel", "stereo_finish_kernel")


def _resource_report(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the flags of stereo.o in csrc/Makefile
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
           "-DNDEBUG", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, "stereo.hip"), "-o", str(tmp_path / "stereo.o")]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning:" not in r.stderr, r.stderr[-4000:]
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


def test_makefile_builds_stereo_with_the_flags_used_here():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bstereo\.hip\b", mk, flags=re.M)
    assert "-O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -fno-gpu-rdc -Wall -Wno-unused-function -DNDEBUG" in mk
    assert not re.search(r"stereo\.o:\s*CXXFLAGS", mk)          # no per-file flags to mirror


def test_stereo_kernels(tmp_path):
    kernels = {k: v for k, v in _resource_report(tmp_path).items() if "stereo_" in k}
    count = lambda s: sum(s in k for k in kernels)      # noqa: E731
    # prepare <REMAP>, path <DIR, ADD> for the five directions, one of everything else
    assert count("stereo_prepare_kernel") == 2 and count("stereo_path_kernel") == 5, sorted(kernels)
    assert len(kernels) == 2 + 5 + 6, sorted(kernels)
    for name, res in sorted(kernels.items()):
        what = (name, "VGPRs", res["VGPRs"], "occupancy", res["Occupancy [waves/SIMD]"], "LDS bytes", res["LDS Size [bytes/block]"], res)
        print(what[:7])
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
        assert int(res["LDS Size [bytes/block]"]) == 0, what
        if any(s in name for s in STREAMING):
            assert int(res["Occupancy [waves/SIMD]"]) == 8 and int(res["VGPRs"]) <= 64, what
        else:
            assert "stereo_path_kernel" in name, name
            # two blocks of ST_UNROLL cost words and sum words in flight, plus addressing: well inside half the file
            assert int(res["VGPRs"]) <= 128, what
