"""The forward plan (csrc/forward_plan.h, built in csrc/binning.hip) through its read-only window ``mgs_debug_forward_plan``
against the plain mirror of its rules (forward_plan_mirror.py), field by field, at every threshold a rule flips on -- and, read
off the sources, that the plan is the only place those rules are written.  No GPU: the window launches nothing."""
import ctypes as C
import itertools
import os
import re

import pytest

import forward_plan_mirror as mirror
from monogs_amd.debug import options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monogs_amd", "csrc")

SIZES = [(16, 16),                   # one tile
         (256, 256),                 # 256 tiles, 8 bits: no bands
         (272, 256),                 # 9 bits, 2 bands
         (640, 480),                 # 11 bits, 5 bands
         (1920, 1080),
         (4080, 4080), (4096, 4080),  # 255 | 256 tile columns: the packed rectangle's byte limit on either side
         (4096, 4096),               # 16 bits
         (4112, 4096),               # 17 bits: no per-tile path
         (2048, 1040)]               # 8 320 tiles: 33 bands
K = 1024
PS = sorted({0, 1, 255, 256, 257} | {c + d for c in (131072, 512 * K, 1 << 21, 1 << 22, 1 << 24) for d in (-1, 0, 1)})
RS_FIXED = {0, 1, 3000} | {c + d for c in (192 * K, 512 * K, 768 * K) for d in (-1, 0, 1)}
OTHERS = [dict(pre_scan=0), dict(scan_small=0), dict(tile_sort_banded=0), dict(dup_slot_major=0), dict(dup_slot_major=1),
          dict(tile_sort_fused=0)]
OPTION_SETS = [{}, dict(radix_scanned=0), dict(radix_scanned=1)] + OTHERS + [dict(radix_scanned=1, **o) for o in OTHERS]


def _plan_indices():
    """{field name in lower case: word index}, in the order the header's enum gives them."""
    text = open(os.path.join(ROOT, "include", "monogs_raster.h")).read()
    body = re.search(r"enum \{\s*MGS_PLAN_P = 0,.*?MGS_PLAN_WORDS\s*\}", text, re.S).group(0)
    names = re.findall(r"\bMGS_PLAN_([A-Z_0-9]+)\b", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names[-1] == "WORDS" and len(set(names)) == len(names)
    return {n.lower(): i for i, n in enumerate(names[:-1])}, len(names) - 1


@pytest.mark.parametrize("opt", OPTION_SETS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_the_window_agrees_with_the_mirror_field_by_field(native_lib, opt):
    lib = native_lib
    idx, words = _plan_indices()
    out = (C.c_uint64 * words)()
    temp_bytes = {}
    points = 0
    with options(**opt):
        for (W, H), P in itertools.product(SIZES, PS):
            path = lib.mgs_binning_path(P, W, H)
            for R, cap, flags in itertools.product(sorted(RS_FIXED | {max(6 * P + d, 0) for d in (-1, 0, 1)}), (0, 1), (0, 1)):
                assert lib.mgs_debug_forward_plan(P, W, H, flags, R, cap, out) == 0
                got = {name: int(out[i]) for name, i in idx.items()}
                key = (got["r"], got["tile_bits"])
                if key not in temp_bytes:
                    temp_bytes[key] = lib.mgs_debug_sort_temp_bytes(*key)
                assert got["two_pass_bytes"] == temp_bytes[key], (P, W, H, R)
                want = mirror.plan(P, W, H, flags, R, bool(cap), opt, got["banded_bytes"], got["two_pass_bytes"])
                assert set(want) | {"banded_bytes", "two_pass_bytes"} == set(got)
                diff = {k: (got[k], v) for k, v in want.items() if got[k] != v}
                assert not diff, (P, W, H, flags, R, cap, diff)
                assert path == got["per_tile"]
                if got["bands"]:
                    assert got["bands_counted"] == got["bands"] and not got["slot_major"]
                    assert got["banded_bytes"] <= got["two_pass_bytes"]
                if got["bands_counted"]:
                    assert got["per_tile"] and got["scan_items"] == 256
                if got["count_digits"]:
                    assert got["bands"] == 0
                points += 1
    assert points >= len(SIZES) * len(PS) * 4 * len(RS_FIXED)


def test_the_cases_reach_every_route(native_lib):
    """The product above is only a check if it holds both answers of every rule: at the default options and with the per-tile
    path forced, each field takes at least two values (banding gives way at a few thousand instances, among others)."""
    idx, words = _plan_indices()
    out = (C.c_uint64 * words)()
    seen = {name: set() for name in idx}
    for opt in ({}, dict(radix_scanned=1)):
        with options(**opt):
            for (W, H), P, R, cap in itertools.product(SIZES, PS, sorted(RS_FIXED), (0, 1)):
                assert native_lib.mgs_debug_forward_plan(P, W, H, cap, R, cap, out) == 0
                for name, i in idx.items():
                    seen[name].add(int(out[i]))
                if (W, H, P, R) == (1920, 1080, 257, 3000) and opt:
                    assert (int(out[idx["bands_counted"]]), int(out[idx["bands"]])) == (32, 0)     # a partial tile per band outweighs 3000 pairs
                if (W, H, P, R) == (1920, 1080, 257, 192 * K) and opt:
                    assert int(out[idx["bands"]]) == 32
    assert not [name for name, vals in seen.items() if len(vals) < 2]


def test_the_window_refuses_null_and_sets_nothing(native_lib):
    assert native_lib.mgs_debug_forward_plan(1000, 640, 480, 0, 5000, 0, None) == 1
    assert b"non-NULL" in native_lib.mgs_last_error()
    out = (C.c_uint64 * 64)()
    assert native_lib.mgs_debug_forward_plan(1000, 0, 480, 0, 5000, 0, out) == 1
    before = native_lib.mgs_debug_last_tile_sort_bands()
    with options(radix_scanned=1):
        assert native_lib.mgs_debug_forward_plan(5000, 640, 480, 0, 200000, 0, out) == 0
    assert native_lib.mgs_debug_last_tile_sort_bands() == before              # the bands of the last emission LAUNCHED


# ---- read off the sources ------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _units():
    return {n: _src(n) for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".h"))}


MOVED_OPTIONS = ("g_opt_scan_small", "g_opt_pre_scan", "g_opt_tile_sort_banded", "g_opt_dup_slot_major", "g_opt_tile_sort_fused")
LAUNCHERS = ("launch_preprocess_forward", "launch_scan", "launch_depth_sort", "launch_duplicate", "launch_emit_banded", "launch_sort",
             "tile_sort_args", "launch_tile_depth_sort", "launch_blend_forward")


def test_the_route_options_are_read_in_the_builder_only():
    files = _units()
    binning = files["binning.hip"]
    start = binning.index("ForwardPlan forward_plan(")
    end = binning.index("\n}\n", binning.index("ForwardPlan ForwardPlan::render(")) + 3
    for name in MOVED_OPTIONS:
        uses = {f: [m.start() for m in re.finditer(r"\b%s\b" % name, text)] for f, text in files.items()}
        uses = {f: at for f, at in uses.items() if at}
        assert set(uses) == {"binning.hip", "common.h", "api.hip"}, (name, sorted(uses))
        assert re.findall(r"[^\n]*\b%s\b[^\n]*" % name, files["common.h"]) and all(
            ln.startswith("extern int ") for ln in re.findall(r"[^\n]*\b%s\b[^\n]*" % name, files["common.h"]))
        assert [files["api.hip"][at - 1] for at in uses["api.hip"]] == ["&"], name                # the option table's row
        definition = re.search(r"^int %s = -?\d+;" % name, binning, re.M)
        assert definition and definition.start() < start
        assert all(start <= at < end for at in uses["binning.hip"] if at != definition.start() + len("int ")), name


def test_common_h_no_longer_declares_the_route_predicates():
    header = re.sub(r"//[^\n]*", "", _src("common.h"))
    for name in ("scan_items", "tile_sort_bands", "tile_sort_bands_render", "depth_sort_payload", "binning_path",
                 "radix_wants_hist", "radix_depth_payload"):
        assert not re.search(r"\b%s\s*\(" % name, header), name
    assert '#include "forward_plan.h"' in _src("common.h")
    for name, text in _units().items():
        if name != "common.h":
            assert '"forward_plan.h"' not in text, name                       # reached through common.h


def test_no_forward_launcher_has_a_defaulted_parameter():
    files = _units()
    for name in LAUNCHERS:
        heads = [m.group(1) for text in files.values()
                 for m in re.finditer(r"^(?:static )?(?:int|TileSortArgs) %s\(([^;{]*)\)\s*[;{]" % name, text, re.M)]
        assert heads, name
        for params in heads:
            assert "=" not in params, (name, params)
            assert params.split(",")[0].strip() == "const ForwardPlan& plan", (name, params)
