"""The scratch layout has one owner, the library (``mgs_debug_scratch_field``, csrc/api.hip): it reproduces the sizes and
offsets recorded from ABI v21 (tests/golden/scratch_layout.json, made by tests/golden/make_golden_scratch_layout.py), no Python
file computes an offset of its own or drives the raw forward beside ``rasterizer.py`` and ``debug.py``, and every knob of
``mgs_debug_set_option`` returns to its default with -1.  No GPU needed."""
import ast
import ctypes as C
import glob
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = sorted(glob.glob(os.path.join(ROOT, "monogs_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "*.py")))
GEOMETRY = ("rec", "depth_key", "depth_alt", "iota", "iota_alt", "perm", "point_offsets", "scan_blocks", "clamped", "rect",
            "rect_sorted", "scan_status", "tile_hist", "sort_temp", "prepare")
BINNING = ("keys_a", "keys_b", "vals_a", "vals_b", "sort_temp", "count", "fwd_masks", "point_list")


def _field(lib, name, P=0, R=0, W=16, H=16):
    off, n = C.c_uint64(0), C.c_uint64(0)
    assert lib.mgs_debug_scratch_field(name.encode(), P, R, W, H, C.byref(off), C.byref(n)) == 0, name
    return [off.value, n.value]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "scratch_layout.json")) as f:
        return json.load(f)


def test_sizes_and_offsets_are_those_of_v21(native_lib, recorded):
    lib = native_lib
    dims = dict(geometry=("P",), image=("W", "H"), binning=("R", "W", "H"), backward=("P",))
    size = dict(geometry=lambda P: lib.mgs_geometry_bytes(P), image=lambda W, H: lib.mgs_image_bytes(W, H),
                binning=lambda R, W, H: lib.mgs_binning_bytes(R, W, H), backward=lambda P: lib.mgs_backward_bytes(P))
    assert len(recorded["geometry"]) == 12 and len(recorded["image"]) == 7 and len(recorded["binning"]) == 56
    for scratch, keys in dims.items():
        for row in recorded[scratch]:
            d = {k: row[k] for k in keys}
            assert size[scratch](**d) == row["bytes"], (scratch, d)
            for member, want in row["fields"].items():
                assert _field(lib, f"{scratch}.{member}", **d) == want, (scratch, member, d)


def test_every_member_has_a_name_and_lies_inside_its_scratch(native_lib):
    lib = native_lib
    P, R, W, H = 5000, 100000, 272, 256
    for scratch, members, total in (("geometry", GEOMETRY, lib.mgs_geometry_bytes(P)),
                                    ("image", ("final_T", "n_contrib", "ranges"), lib.mgs_image_bytes(W, H)),
                                    ("binning", BINNING, lib.mgs_binning_bytes(R, W, H)),
                                    ("backward", ("grad_acc", "tau_part", "tau"), lib.mgs_backward_bytes(P))):
        spans = [_field(lib, f"{scratch}.{m}", P, R, W, H) for m in members]
        for (off, n), m in zip(spans, members):
            assert off % (64 if scratch == "backward" else 256) == 0 and off + n + 256 <= total, (scratch, m)
        real = [s for s, m in zip(spans, members) if m != "point_list"]
        assert real == sorted(real) and all(a[0] + a[1] <= b[0] for a, b in zip(real, real[1:])), scratch
    # the alias follows the tile sort's pass count: 256 tiles = one pass = the b buffers, 272 tiles = two passes = a
    assert _field(lib, "binning.point_list", R=R, W=256, H=256) == _field(lib, "binning.vals_b", R=R, W=256, H=256)
    assert _field(lib, "binning.point_list", R=R, W=272, H=256) == _field(lib, "binning.vals_a", R=R, W=272, H=256)
    base = 1 << 20
    assert lib.mgs_backward_tau(base, P) - base == _field(lib, "backward.tau", P)[0]


@pytest.mark.parametrize("name", ["geometry.nothing", "geometry", "", "rec", "attic.rec", "binning.point_list.x", "geometry.end"])
def test_an_unknown_field_is_an_error_with_a_message(native_lib, name):
    off, n = C.c_uint64(7), C.c_uint64(7)
    assert native_lib.mgs_debug_scratch_field(name.encode(), 10, 10, 16, 16, C.byref(off), C.byref(n)) != 0
    assert b"unknown field" in native_lib.mgs_last_error()
    assert (off.value, n.value) == (7, 7)


# ---- no second statement of the layout, no second raw driver ------------------------------------------------------------------

RAW = ("mgs_forward_preprocess", "mgs_forward_render", "mgs_forward_render_capacity", "mgs_forward_capacity", "mgs_backward")


def _trees():
    assert len(SOURCES) > 100
    for path in SOURCES:
        with open(path) as f:
            text = f.read()
        yield os.path.relpath(path, ROOT), text, ast.parse(text)


def test_only_the_rasteriser_and_debug_call_the_raw_forward_and_backward():
    """Every place that takes one of the entry points off the library handle, called there or not.  Two tests stay beside the
    two drivers, each for one argument edge no driver produces: a render of an empty map with geometry == NULL, and a backward
    with one of the two image pointers nulled by a wrapper around the rasteriser's own call."""
    users = {}
    for path, _, tree in _trees():
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and node.attr in RAW:
                users.setdefault(path, set()).add(node.attr)
    assert users == {"monogs_amd/rasterizer.py": {"mgs_forward_preprocess", "mgs_forward_render", "mgs_forward_capacity", "mgs_backward"},
                     "monogs_amd/debug.py": {"mgs_forward_preprocess", "mgs_forward_render", "mgs_forward_render_capacity", "mgs_backward"},
                     "tests/test_gpu_features.py": {"mgs_forward_render", "mgs_forward_render_capacity"},
                     "tests/test_gpu_blend_backward_split.py": {"mgs_backward"}}


def test_no_python_file_rounds_offsets_up_for_itself():
    """An ``_au`` / ``_al``-style helper (round up to a multiple of 256) is how a copy of the layout starts.  The one that stands:
    the rasteriser's arena sizing, which rounds the library's three ``*_bytes`` results."""
    round_up = re.compile(r"\+\s*255\s*\)\s*//\s*256|\+\s*a\s*-\s*1\s*\)\s*//\s*a\s*\*\s*a|\bdef _a[ul]\(")
    found = {path for path, text, _ in _trees() if round_up.search(text) and path != "tests/test_scratch_layout.py"}
    assert found == {"monogs_amd/rasterizer.py"}
    with open(os.path.join(ROOT, "monogs_amd", "rasterizer.py")) as f:
        uses = set(re.findall(r"\b_al\(([\w.]+)", f.read()))
    assert uses == {"n", "lib.mgs_geometry_bytes", "lib.mgs_image_bytes", "lib.mgs_backward_bytes"}


def test_nobody_else_indexes_the_rasterisers_saved_tensors():
    """Positional knowledge of the autograd node (ten saved tensors, the arena and the binning scratch last) stays in
    rasterizer.py: everything else asks ``forward_scratch(color)``."""
    for path, text, tree in _trees():
        if path == "monogs_amd/rasterizer.py":
            continue
        for node in ast.walk(tree):
            if isinstance(node, ast.Subscript):
                v = node.value
                name = v.attr if isinstance(v, ast.Attribute) else v.id if isinstance(v, ast.Name) else ""
                assert name not in ("saved_tensors", "saved"), (path, node.lineno)
        for attr in ("geom_off", "img_off"):                 # a node's offsets are read through the handle
            assert not re.search(r"\bfn\.%s\b|grad_fn\.%s\b" % (attr, attr), text), (path, attr)


# ---- the option table ---------------------------------------------------------------------------------------------------------

def _option_names():
    with open(os.path.join(ROOT, "include", "monogs_raster.h")) as f:
        text = f.read()
    comment = text[:text.index("int mgs_debug_set_option(")].rsplit("/* TEST USE ONLY", 1)[1]
    names = re.findall(r'"([a-z0-9_]+)"', comment)
    assert len(set(names)) == 13, names
    return sorted(set(names))


def test_minus_one_is_accepted_by_every_option_the_header_names(native_lib):
    for name in _option_names():
        assert native_lib.mgs_debug_set_option(name.encode(), -1) == 0, name
    assert native_lib.mgs_debug_set_option(b"no_such_option", -1) == 1
    assert native_lib.mgs_debug_set_option(b"no_such_option", 0) == 1
    assert b"unknown option" in native_lib.mgs_last_error()


def test_the_binning_path_follows_radix_scanned_and_minus_one_restores_it(native_lib):
    lib = native_lib
    small, large = 5000, 600000                     # the depth sort takes the counted-tiles path above 512 k Gaussians
    try:
        assert (lib.mgs_binning_path(small, 640, 480), lib.mgs_binning_path(large, 640, 480)) == (0, 1)
        for value, want in ((0, (0, 0)), (1, (1, 1)), (-1, (0, 1)), (1, (1, 1)), (-7, (0, 1))):
            assert lib.mgs_debug_set_option(b"radix_scanned", value) == 0
            assert (lib.mgs_binning_path(small, 640, 480), lib.mgs_binning_path(large, 640, 480)) == want, value
    finally:
        lib.mgs_debug_set_option(b"radix_scanned", -1)


def test_the_options_context_manager_restores_with_minus_one(monkeypatch):
    from monogs_amd import _lib, debug
    calls = []

    class Lib:
        def mgs_debug_set_option(self, name, value):
            calls.append((name, value))
            return 0
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    with pytest.raises(ZeroDivisionError):
        with debug.options(pre_scan=0, radix_scanned=1):
            assert calls == [(b"pre_scan", 0), (b"radix_scanned", 1)]
            1 / 0
    assert calls[2:] == [(b"radix_scanned", -1), (b"pre_scan", -1)]
