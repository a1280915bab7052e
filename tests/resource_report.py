"""The compiler's resource report of one unit of monogs_amd/csrc for gfx950 (no GPU needed), for the test_*_resources.py files.

The unit is compiled with the command csrc/Makefile runs for it -- taken from a dry run of make, so the common and the per-file
flags are the Makefile's, by the extraction tools/kernel_identity.py uses -- with `-c` widened to
`--cuda-device-only -Rpass-analysis=kernel-resource-usage -c`."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")

_spec = importlib.util.spec_from_file_location("kernel_identity", os.path.join(ROOT, "tools", "kernel_identity.py"))
_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_tool)

_reports = {}           # unit -> (kernels, stderr): several test files ask about the same unit


def compile_commands(unit):
    """The compile commands (argument lists) a dry run of csrc/Makefile yields for `unit`, e.g. "blend.hip"."""
    return _tool.compile_commands(ROOT, unit)


def resource_report(unit, tmp_path):
    """({kernel symbol: {field: value}}, the compiler's stderr) of `unit`; the fields are the remark's: "VGPRs", "TotalSGPRs",
    "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", ..."""
    if unit not in _reports:
        (cmd,) = compile_commands(unit)
        at = cmd.index("-c")
        cmd[at:at + 1] = ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c"]
        cmd[cmd.index("-o") + 1] = str(tmp_path / (unit[:-len(".hip")] + ".o"))
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
        _reports[unit] = (kernels, r.stderr)
    return _reports[unit]
