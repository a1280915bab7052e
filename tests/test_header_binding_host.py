"""The binding is derived from include/monogs_raster.h by monogs_amd/_header.py: the reader against hand-written ctypes
expectations on a small header, its refusals, and the real header against regexes of this file and against the C compiler."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from monogs_amd import _header, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monogs_raster.h")

SYNTHETIC_HEAD = """/* a block comment
   over two lines; with a semicolon and a brace { */
#ifndef SYN_H
#define SYN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define MGS_ONE 1u
#define MGS_HALF 0.5f     // a line comment
#define MGS_BIG ((1 << 20) + MGS_ONE)
#define MGS_MASK (MGS_BIG | 0x10)
typedef struct syn_point {
    int32_t x, y;         /* several declarators on one line */
    float w[3];
    const float* data;
    uint8_t** rows;
    double scale;
    uint64_t n;
} syn_point;
typedef struct SynParamsTag { float a; int32_t b; } SynParams;
enum { MGS_E_A = 0, MGS_E_B, MGS_E_C = 7, MGS_E_D,
       MGS_E_WORDS };
int syn_version(void);
const char* syn_name(void);
float* syn_data(const syn_point* p, int32_t n);
size_t syn_bytes(unsigned long long n, const char* tag, const uint64_t* const* table,
                 SynParams* params, void* stream);
"""
SYNTHETIC_TAIL = """#ifdef __cplusplus
}
#endif
#endif /* SYN_H */
"""


def test_the_reader_on_a_small_header():
    h = _header.parse(SYNTHETIC_HEAD + SYNTHETIC_TAIL, "syn.h")
    assert list(h.structs) == ["SynPoint", "SynParams"]
    point, params = h.structs["SynPoint"], h.structs["SynParams"]
    assert issubclass(point, C.Structure) and point.__name__ == "SynPoint"
    assert point._fields_ == [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_float * 3), ("data", C.c_void_p), ("rows", C.c_void_p),
                              ("scale", C.c_double), ("n", C.c_uint64)]
    assert params._fields_ == [("a", C.c_float), ("b", C.c_int32)]
    assert C.sizeof(point) == 4 + 4 + 12 + 4 + 8 + 8 + 8 + 8          # x, y, w, padding, data, rows, scale, n
    assert h.functions == {
        "syn_version": (C.c_int, []),
        "syn_name": (C.c_char_p, []),
        "syn_data": (C.c_void_p, [C.POINTER(point), C.c_int32]),
        "syn_bytes": (C.c_size_t, [C.c_ulonglong, C.c_char_p, C.c_void_p, C.POINTER(params), C.c_void_p]),
    }
    assert vars(h.constants) == dict(MGS_ONE=1, MGS_HALF=0.5, MGS_BIG=(1 << 20) + 1, MGS_MASK=(1 << 20) + 1 | 16,
                                     MGS_E_A=0, MGS_E_B=1, MGS_E_C=7, MGS_E_D=8, MGS_E_WORDS=9)
    assert isinstance(h.constants.MGS_ONE, int) and isinstance(h.constants.MGS_HALF, float)
    p = point(x=1, y=2, n=3)                                            # keyword construction, as MgsKeyframeParams(**kw)
    assert (p.x, p.y, p.n) == (1, 2, 3) and point.from_buffer_copy(bytes(p)).y == 2


@pytest.mark.parametrize("extra, offending, word", [
    ("int syn_ok(int32_t a);\nint syn_bad(int32_t a,\n            widget_t w);\n", 2, "widget_t"),        # an unknown type
    ("typedef struct syn_open {\n    int32_t a;\n", 0, "syn_open"),                                          # an unterminated struct
    ("int syn_ok(int32_t a);\nint32_t syn_counter;\n", 1, "syn_counter"),                                    # a stray statement
    ("typedef struct syn_m {\n    int32_t a;\n    float m[4][4];\n} syn_m;\n", 2, "m[4][4]"),                 # a declarator the grammar lacks
    ("int syn_cb(int (*cb)(int));\n", 0, "syn_cb"),                                                           # and another
    ("#define MGS_LATE (MGS_LATER + 1)\n", 0, "MGS_LATER"),                                                   # a define before its operand
])
def test_the_reader_refuses_what_it_does_not_know(extra, offending, word):
    line = SYNTHETIC_HEAD.count("\n") + 1 + offending
    with pytest.raises(_header.HeaderError) as e:
        _header.parse(SYNTHETIC_HEAD + extra + SYNTHETIC_TAIL, "syn.h")
    assert str(e.value).startswith(f"syn.h:{line}: ") and word in str(e.value), str(e.value)


def _stripped_header():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_the_binding_declares_what_the_header_declares():
    text = _stripped_header()
    assert set(_lib.SIGNATURES) == set(re.findall(r"\b(mgs_[a-z0-9_]+)\s*\(", text)) and len(_lib.SIGNATURES) > 90
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        assert isinstance(argtypes, list) and restype in (C.c_int, C.c_int32, C.c_size_t, C.c_char_p, C.c_void_p), name
    assert _lib.SIGNATURES is _header.read().functions and _lib.ABI_VERSION == _lib.H.MGS_ABI_VERSION
    assert _lib.FLAG_EXCLUSIVE_DEVICE == 1 and _lib.FLAG_INTRINSICS_GRAD == 2 and _lib.c_float_p is C.c_void_p
    assert _lib.MgsTiming(scan_ms=2.0).as_dict()["scan_ms"] == 2.0 and len(_lib.MgsTiming().as_dict()) == 9


def test_every_constant_equals_its_define():
    text = _stripped_header()
    defines = dict(re.findall(r"^#define (MGS_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M))
    enum = re.findall(r"\b(MGS_PLAN_\w+)\b", re.search(r"\benum\s*\{(.*?)\}", text, flags=re.S).group(1))
    assert set(vars(_lib.H)) == set(defines) | set(enum) and len(defines) > 35
    expressions = {}
    for name, value in defines.items():
        if re.fullmatch(r"\d+u?", value):
            assert getattr(_lib.H, name) == int(value.rstrip("u")) and isinstance(getattr(_lib.H, name), int), name
        elif re.fullmatch(r"\d+\.\d+f?", value):
            assert getattr(_lib.H, name) == float(value.rstrip("f")), name
        else:
            expressions[name] = value
    assert expressions == {"MGS_MAX_GAUSSIANS": "((1 << 26) - 1)"} and _lib.H.MGS_MAX_GAUSSIANS == 2 ** 26 - 1
    # the anonymous enum counts up from MGS_PLAN_P = 0 and ends at MGS_PLAN_WORDS, the number of words before it
    assert [getattr(_lib.H, n) for n in enum] == list(range(len(enum))) and enum[0] == "MGS_PLAN_P"
    assert enum[-1] == "MGS_PLAN_WORDS" and _lib.H.MGS_PLAN_WORDS == len(enum) - 1 == 30


C_NAMES = dict(mgs_camera="MgsCamera", mgs_timing="MgsTiming", MgsKeyframeParams="MgsKeyframeParams",
               MgsPseudoDepthParams="MgsPseudoDepthParams", MgsFramePrepare="MgsFramePrepare", MgsStereo="MgsStereo",
               mgs_tsdf_volume="MgsTsdfVolume", mgs_tsdf_frame="MgsTsdfFrame", MgsMeshRender="MgsMeshRender")


def _host_compiler():
    for name, flags in (("cc", []), ("hipcc", ["-x", "c"]), ("/opt/rocm/bin/hipcc", ["-x", "c"])):      # hipcc: as a plain C compiler
        if shutil.which(name):
            return [shutil.which(name)] + flags
    return None


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every offsetof, as the host C compiler lays the header's structs out, against the derived ctypes classes."""
    assert set(re.findall(r"\}\s*(\w+)\s*;", _stripped_header())) == set(C_NAMES)
    assert set(C_NAMES.values()) == set(_header.read().structs)
    compiler = _host_compiler()
    if compiler is None:
        pytest.skip("no host C compiler on this machine")
    lines = ['#include <stdio.h>', '#include "monogs_raster.h"', "int main(void) {"]
    for c_name, py_name in C_NAMES.items():
        lines.append(f'    printf("{py_name} %zu\\n", sizeof({c_name}));')
        for field, _ in getattr(_lib, py_name)._fields_:
            lines.append(f'    printf("{py_name}.{field} %zu\\n", offsetof({c_name}, {field}));')
    source, program = tmp_path / "layout.c", tmp_path / "layout"
    source.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run(compiler + ["-I", os.path.dirname(HEADER), str(source), "-o", str(program)], check=True, capture_output=True)
    measured = dict(line.split() for line in subprocess.run([str(program)], check=True, capture_output=True, text=True).stdout.splitlines())
    expected = {}
    for py_name in C_NAMES.values():
        cls = getattr(_lib, py_name)
        expected[py_name] = str(C.sizeof(cls))
        expected.update({f"{py_name}.{field}": str(getattr(cls, field).offset) for field, _ in cls._fields_})
    assert measured == expected and len(expected) > 100
