"""The image-metrics kernels (csrc/metrics.hip) are streaming kernels bound by memory: the compiler's resource report for
gfx950 (no GPU needed) must show no scratch, full occupancy (8 waves per SIMD, i.e. at most 64 VGPRs) and no LDS beyond the
48 bytes of the workgroup sum (four doubles + four counts)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")


def _resource_report(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the flags of metrics.o in csrc/Makefile
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
           "-DNDEBUG", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, "metrics.hip"), "-o", str(tmp_path / "metrics.o")]
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


def test_makefile_builds_metrics_with_the_flags_used_here():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bmetrics\.hip\b", mk, flags=re.M)
    assert "-O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -fno-gpu-rdc -Wall -Wno-unused-function -DNDEBUG" in mk
    assert not re.search(r"metrics\.o:\s*CXXFLAGS", mk)          # no per-file flags to mirror


def test_metrics_kernels_stream(tmp_path):
    kernels = _resource_report(tmp_path)
    main = {k: v for k, v in kernels.items() if "metrics_kernel" in k}
    fin = {k: v for k, v in kernels.items() if "metrics_finalize_kernel" in k}
    assert len(main) == 2 and len(fin) == 1, sorted(kernels)        # <VEC = true>, <VEC = false>
    for name, res in {**main, **fin}.items():
        what = (name, "VGPRs", res["VGPRs"], "LDS bytes", res["LDS Size [bytes/block]"], res)
        print(what[:5])
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
        assert int(res["Occupancy [waves/SIMD]"]) == 8 and int(res["VGPRs"]) <= 64, what       # built: 52 (vector), 26 (scalar), 20
        assert int(res["LDS Size [bytes/block]"]) <= 48, what                                  # built: 48
