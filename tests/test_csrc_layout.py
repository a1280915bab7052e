"""What the HIP units share is stated once: the wave primitives in ``csrc/wave_ops.h`` (reached through ``common.h``), the
order-preserving float/int map and the scratch cursor in ``common.h``.  And what a unit is: a file with kernels or entry points
is a ``.hip`` named in the Makefile's ``SRCS``, a header is what units include.  Reads the sources only; no GPU, no library."""
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


def _makefile_srcs():
    with open(os.path.join(CSRC, "Makefile")) as f:
        (srcs,) = re.findall(r"^SRCS\s*=\s*(.+)$", f.read(), re.M)
    return srcs.split()


def _the_units():
    """The ``*.hip`` files, which are exactly the Makefile's ``SRCS``."""
    units, srcs = _sources("*.hip"), _makefile_srcs()
    assert len(srcs) == len(set(srcs)), srcs
    assert set(units) == set(srcs), set(units) ^ set(srcs)
    assert len(units) >= 25
    return units


def test_the_units_are_the_makefiles_srcs():
    _the_units()


def test_kernels_and_entry_points_live_in_units():
    headers = _sources("*.h")
    assert not [name for name, text in headers.items() if 'extern "C"' in text]
    assert {name for name, text in headers.items() if "__global__" in text} == {"common.h"}      # its two static fill kernels
    assert len(re.findall(r"__global__", headers["common.h"])) == 2
    for name, text in {**_sources("*.hip"), **headers}.items():
        assert not [inc for inc in re.findall(r'^\s*#\s*include\s+["<]([^">]+)[">]', text, re.M) if inc.endswith(".hip")], name


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
    units = _the_units()
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
