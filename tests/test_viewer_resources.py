"""The viewer kernels (csrc/viewer.hip) compile for gfx950 with the Makefile's flags, without warnings and without scratch: the
ellipsoid walk keeps a pixel's colour, hit and "open" state per lane and fetches a candidate's record with scalar loads, and a
spill there would be a design error.  The register, occupancy and LDS figures are printed; DESIGN.md quotes the walk's.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")
KERNELS = ("viewer_ellipsoids_kernel", "viewer_empty_kernel", "viewer_lines_kernel", "viewer_max_kernel", "viewer_compose_kernel")


def _resource_report(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the flags of viewer.o in csrc/Makefile
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
           "-DNDEBUG", "-fno-slp-vectorize", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, "viewer.hip"), "-o", str(tmp_path / "viewer.o")]
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


def test_makefile_builds_the_viewer_with_the_flags_used_here():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bviewer\.hip\b", mk, flags=re.M)
    assert "-O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -fno-gpu-rdc -Wall -Wno-unused-function -DNDEBUG" in mk
    assert re.search(r"^\$\(OUT\)/viewer\.o:\s*CXXFLAGS \+= -fno-slp-vectorize\s*$", mk, flags=re.M)


def test_viewer_kernels_do_not_spill(tmp_path):
    kernels = _resource_report(tmp_path)
    for want in KERNELS:
        found = {k: v for k, v in kernels.items() if want in k}
        assert len(found) == 1, (want, sorted(kernels))
        (name, res), = found.items()
        what = (want, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "waves/SIMD", res["Occupancy [waves/SIMD]"],
                "LDS bytes", res["LDS Size [bytes/block]"])
        print(what)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
        assert int(res["LDS Size [bytes/block]"]) == 0, what
    # what only the viewer kernels and the shared clears live in this file
    assert all(any(w in k for w in KERNELS) or "zero_fill" in k for k in kernels), sorted(kernels)
