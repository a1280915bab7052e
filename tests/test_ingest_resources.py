"""The frame-ingest kernels (csrc/ingest.hip) are streaming kernels and a 3x3 stencil, bound by memory: the compiler's resource
report for gfx950 (no GPU needed) must show no scratch, full occupancy (8 waves per SIMD, i.e. at most 64 VGPRs) and no LDS for
every one of them, on the vector and on the scalar route."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")


def _resource_report(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the flags of ingest.o in csrc/Makefile
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
           "-DNDEBUG", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, "ingest.hip"), "-o", str(tmp_path / "ingest.o")]
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


def test_makefile_builds_ingest_with_the_flags_used_here():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bingest\.hip\b", mk, flags=re.M)
    assert "-O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -fno-gpu-rdc -Wall -Wno-unused-function -DNDEBUG" in mk
    assert not re.search(r"ingest\.o:\s*CXXFLAGS", mk)          # no per-file flags to mirror


def test_ingest_kernels_stream(tmp_path):
    kernels = {k: v for k, v in _resource_report(tmp_path).items() if "ingest_" in k}
    count = lambda s: sum(s in k for k in kernels)      # noqa: E731
    # prepare <VEC, REMAP>, intensity <VEC>, threshold <VEC>
    assert (count("ingest_prepare_kernel"), count("ingest_intensity_kernel"), count("ingest_threshold_kernel")) == (4, 2, 2), sorted(kernels)
    assert len(kernels) == 8, sorted(kernels)
    for name, res in kernels.items():
        what = (name, "VGPRs", res["VGPRs"], "LDS bytes", res["LDS Size [bytes/block]"], res)
        print(what[:5])
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
        # built: prepare 47 / 59 / 18 / 38, intensity 62 (vector) / 46, threshold 10 / 4
        assert int(res["Occupancy [waves/SIMD]"]) == 8 and int(res["VGPRs"]) <= 64, what
        assert int(res["LDS Size [bytes/block]"]) == 0, what
