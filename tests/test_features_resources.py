"""The feature kernels (csrc/features.hip) keep a chunk of C accumulators (forward) or C upstream gradients (backward) per lane.
The compiler's resource report for gfx950 (no GPU needed) must show no scratch for any instantiation: a spilled chunk is a
wrong choice of C, not something to accept.  The register, occupancy and LDS figures are printed; DESIGN.md section 3 quotes
the ones that were built."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")


def _resource_report(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the flags of features.o in csrc/Makefile
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
           "-DNDEBUG", "-fno-slp-vectorize", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, "features.hip"), "-o", str(tmp_path / "features.o")]
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


def test_makefile_builds_features_with_the_flags_used_here():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bfeatures\.hip\b", mk, flags=re.M)
    assert "-O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -fno-gpu-rdc -Wall -Wno-unused-function -DNDEBUG" in mk
    assert re.search(r"^\$\(OUT\)/features\.o:\s*CXXFLAGS \+= -fno-slp-vectorize\s*$", mk, flags=re.M)


def test_feature_kernels_do_not_spill(tmp_path):
    kernels = _resource_report(tmp_path)
    fwd = {k: v for k, v in kernels.items() if "features_forward_kernel" in k}
    bwd = {k: v for k, v in kernels.items() if "features_backward_kernel" in k}
    empty = {k: v for k, v in kernels.items() if "features_empty_kernel" in k}
    assert len(fwd) == 3 and len(bwd) == 3 and len(empty) == 1, sorted(kernels)        # C = 4, 8, 16 each way
    for name, res in {**fwd, **bwd, **empty}.items():
        what = (name, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "waves/SIMD", res["Occupancy [waves/SIMD]"],
                "LDS bytes", res["LDS Size [bytes/block]"])
        print(what)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
    # built (VGPRs / waves per SIMD): forward C = 4: 23 / 8, C = 8: 31 / 8, C = 16: 47 / 8; backward 24 / 8, 32 / 8, 48 / 8;
    # no LDS anywhere.  (C = 32, not built: 80 and 74 VGPRs, 6 waves, the forward at 106 SGPRs.)
