"""The keyframe-window kernels in the compiler's resource report for gfx950 (no GPU needed): none of them spills to
private-memory scratch -- the covisibility and the decision kernel index pointer tables in their kernel arguments by lane, which
must stay loads from the argument segment -- and the LDS of the median's kernels is what csrc/kfwindow.hip says: one histogram of
2048 buckets (8192 bytes) per workgroup of the counting launch, the summed histogram plus 256 scan words (9216 bytes) in the
selecting launch."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")


def _resource_report(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # the flags of kfwindow.o in csrc/Makefile
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
           "-DNDEBUG", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, "kfwindow.hip"), "-o", str(tmp_path / "kfwindow.o")]
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


def test_makefile_builds_kfwindow_with_the_flags_used_here():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkfwindow\.hip\b", mk, flags=re.M)
    assert "-O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -fno-gpu-rdc -Wall -Wno-unused-function -DNDEBUG" in mk
    assert not re.search(r"kfwindow\.o:\s*CXXFLAGS", mk)      # no per-file flags to mirror


def test_kfwindow_kernels_use_no_scratch_and_the_recorded_lds(tmp_path):
    kernels = _resource_report(tmp_path)
    pick = lambda s: {k: v for k, v in kernels.items() if s in k}  # noqa: E731
    hist, select = pick("median_hist_kernel"), pick("median_select_kernel")
    covis, decide = pick("covisibility_kernel"), pick("keyframe_decide_kernel")
    assert len(hist) == 3 and len(select) == 3 and len(covis) == 1 and len(decide) == 1, sorted(kernels)     # <PASS> 0, 1, 2
    for name, res in {**hist, **select, **covis, **decide}.items():
        assert int(res["ScratchSize [bytes/lane]"]) == 0, (name, res)
        assert int(res["Occupancy [waves/SIMD]"]) >= 4, (name, res)
    for name, res in hist.items():
        assert int(res["LDS Size [bytes/block]"]) == 2048 * 4, (name, res)
    for name, res in select.items():
        assert int(res["LDS Size [bytes/block]"]) == (2048 + 256) * 4, (name, res)
    for name, res in {**covis, **decide}.items():
        assert int(res["LDS Size [bytes/block]"]) <= 2048, (name, res)
