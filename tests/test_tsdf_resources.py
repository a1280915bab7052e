"""The TSDF kernels (csrc/tsdf.hip) are one lane per voxel with a handful of live values; the emit kernels unroll seven edges and six
tetrahedra.  The compiler's resource report for gfx950 (no GPU needed) must show no scratch for any kernel of the file.  The register,
occupancy and LDS figures are printed; DESIGN.md ("TSDF fusion and mesh extraction") quotes them."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")
KERNELS = ("tsdf_integrate_kernel", "tsdf_classify_kernel", "tsdf_cells_kernel", "tsdf_edges_kernel", "tsdf_scan_local_kernel",
           "tsdf_scan_blocks_kernel", "tsdf_emit_vertices_kernel", "tsdf_emit_triangles_kernel")


def _resource_report(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the flags of tsdf.o in csrc/Makefile (the common ones: the file has no line of its own there)
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
           "-DNDEBUG", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, "tsdf.hip"), "-o", str(tmp_path / "tsdf.o")]
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


def test_makefile_builds_tsdf_with_the_flags_used_here():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\btsdf\.hip\b", mk, flags=re.M)
    assert "-O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -fno-gpu-rdc -Wall -Wno-unused-function -DNDEBUG" in mk
    assert not re.search(r"^\$\(OUT\)/tsdf\.o:", mk, flags=re.M)                       # no flags of its own


def test_tsdf_kernels_do_not_spill(tmp_path):
    kernels = {k: v for k, v in _resource_report(tmp_path).items() if "tsdf_" in k}
    for want in KERNELS:
        assert sum(1 for k in kernels if want in k) == 1, (want, sorted(kernels))
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for name, res in kernels.items():
        what = (name, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "waves/SIMD", res["Occupancy [waves/SIMD]"],
                "LDS bytes", res["LDS Size [bytes/block]"])
        print(what)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
        assert int(res["Occupancy [waves/SIMD]"]) >= 4, what           # one-lane-per-voxel streaming: latency is hidden by waves
    # the only LDS is the scans' per-wave totals: 4 words, and 16 double words
    lds = {k: int(v["LDS Size [bytes/block]"]) for k, v in kernels.items()}
    assert all(b == 0 for k, b in lds.items() if "scan" not in k), lds
    assert all(b <= 128 for b in lds.values()), lds
