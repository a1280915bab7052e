"""What the HIP units share is stated once: the wave primitives in ``csrc/wave_ops.h`` (reached through ``common.h``), the
order-preserving float/int map and the scratch cursor in ``common.h``.  Reads the sources only; no GPU, no library."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")


def _sources(pattern):
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, pattern))):
        with open(path) as f:
            out[os.path.basename(path)] = f.read()
    return out


def test_the_xor_butterfly_is_written_in_wave_ops_only():
    files = {**_sources("*.hip"), **_sources("*.h")}
    assert len(files) >= 25
    assert {name for name, text in files.items() if "__shfl_xor" in text} == {"wave_ops.h"}


def test_ord2f_is_defined_once():
    files = {**_sources("*.hip"), **_sources("*.h")}
    defs = [(name, m.group(0)) for name, text in files.items() for m in re.finditer(r"\bfloat\s+\w*ord2f\s*\(\s*int32_t", text)]
    assert [name for name, _ in defs] == ["common.h"], defs
    assert not [name for name, text in files.items() if re.search(r"\b\w+_ord2f\b", text)]


def test_no_unit_pastes_the_bump_allocator():
    """``align_up(`` with a ``take`` lambda behind it is how the five copies of the allocator looked."""
    lam = re.compile(r"align_up\(.{0,400}?auto\s+take\s*=\s*\[|auto\s+take\s*=\s*\[[^\n]*align_up\(", re.S)
    units = _sources("*.hip")
    assert len(units) == 21
    assert not [name for name, text in units.items() if lam.search(text)]


def test_every_unit_reaches_wave_ops_through_common():
    units, headers = _sources("*.hip"), _sources("*.h")
    includes = lambda text: set(re.findall(r'^#include\s+"([^"]+)"', text, re.M))  # noqa: E731
    assert "wave_ops.h" in includes(headers["common.h"])
    for name, text in units.items():
        assert "common.h" in includes(text), name
        assert "wave_ops.h" not in includes(text), name
    for name, text in headers.items():
        if name not in ("common.h", "wave_ops.h"):
            assert "wave_ops.h" not in includes(text), name
