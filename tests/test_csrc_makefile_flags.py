"""The flags csrc/Makefile compiles each unit with, read off a dry run of make (the command the test_*_resources.py files and
tools/kernel_identity.py compile with): the common set for every unit, and per unit exactly the extras recorded here -- a flag
that appears or disappears changes the code generated for the kernels those files hold to their register and LDS budgets."""
import os
import re

import pytest

from resource_report import CSRC, compile_commands

COMMON = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function", "-DNDEBUG"]
BLEND = ["-fno-slp-vectorize", "-Wno-inline-asm"]         # scalar blend loops; the forward clobbers M0 on purpose
EXTRA = {
    "tsdf": [], "stereo": [], "labels": [], "ingest": [], "ssim": [], "metrics": [], "kfwindow": [],
    "pose": [], "gauss_newton": [], "object_motion": [], "mesh_render": [],
    "features": ["-fno-slp-vectorize"], "viewer": ["-fno-slp-vectorize"],      # alpha as the blend forms it: the same code generation
    "pose_tangent": ["-fno-slp-vectorize"],                                    # the tangent blend: alpha as features.hip forms it
    "preprocess": ["-ffp-contract=off"],                                       # the geometry that decides integers
    "blend": BLEND, "blend_stats": BLEND,
}


@pytest.mark.parametrize("unit", sorted(EXTRA))
def test_makefile_compiles_the_unit_with_the_recorded_flags(unit):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\b" + unit + r"\.hip\b", mk, flags=re.M)       # part of the library
    cmds = compile_commands(unit + ".hip")
    assert len(cmds) == 1, cmds
    cmd = cmds[0]
    assert cmd[cmd.index("-c") + 1] == unit + ".hip" and cmd[cmd.index("-o") + 1].endswith("/" + unit + ".o"), cmd
    flags = [f for i, f in enumerate(cmd[1:], 1) if f not in ("-c", "-o") and cmd[i - 1] not in ("-c", "-o")]
    assert [f for f in flags if f in COMMON] == COMMON, cmd
    assert [f for f in flags if f not in COMMON] == EXTRA[unit], cmd
