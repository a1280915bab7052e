#!/usr/bin/env python3
"""Writes tests/golden/scratch_layout.json: the sizes and the sub-buffer offsets of the rasteriser's four scratch buffers as
ABI v21 had them, the last version whose layout was also written down as Python arithmetic.

The sizes are what the library's `mgs_*_bytes` return.  The offsets and lengths are that arithmetic, frozen here as it stood
in monogs_amd/debug.py (forward_tables), tests/test_gpu_pre_scan.py and tests/test_gpu_blend_prepare.py (_Abi) at v21; it
is kept nowhere else.  tests/test_scratch_layout.py holds `mgs_debug_scratch_field` of every later library against the
file.  Run with a library of ABI v21 (MGS_LIB_PATH) to regenerate; a layout that is MEANT to move gets a new recording made
from the library's own export instead."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

# scan-block (256 / 2048) and one-launch-scan (131 072) boundaries
PS = (0, 1, 255, 256, 257, 2047, 2048, 2049, 5000, 131072, 131073, 2000000)
RS = (0, 1, 63, 64, 65, 4096, 100000, 5271297)
# 256 x 256: 256 tiles, 8 tile bits, one sort pass, result in the b buffers; 272 x 256: 272 tiles, 9 bits, two passes, in a
WHS = ((16, 16), (17, 33), (256, 256), (272, 256), (640, 480), (1200, 680), (1920, 1080))
TAU_SLOTS = 256          # csrc/common.h at v21


def _au(v, a=256):
    return (v + a - 1) // a * a


def geometry(lib, P):
    o = _au(P * 64)
    o_rect = o + 6 * _au(P * 4) + _au(((P + 255) // 256 + 64) * 4) + _au(P * 4)
    return dict(P=P, bytes=lib.mgs_geometry_bytes(P),
                fields=dict(rec=[0, P * 64], depth_key=[o, P * 4], perm=[o + 4 * _au(P * 4), P * 4],
                            rect=[o_rect, P * 8], rect_sorted=[o_rect + _au(P * 8), P * 8]))


def image(lib, W, H):
    HW, ntiles = H * W, ((W + 15) // 16) * ((H + 15) // 16)
    return dict(W=W, H=H, bytes=lib.mgs_image_bytes(W, H),
                fields=dict(final_T=[0, HW * 4], n_contrib=[_au(HW * 4), HW * 4], ranges=[2 * _au(HW * 4), ntiles * 8]))


def binning(lib, R, W, H):
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    tile_bits = max(1, (ntiles - 1).bit_length())
    in_b = ((tile_bits + 7) // 8) % 2 == 1
    return dict(R=R, W=W, H=H, bytes=lib.mgs_binning_bytes(R, W, H),
                fields=dict(point_list=[(3 if in_b else 2) * _au(max(R, 1) * 4), R * 4]))


def backward(lib, P):
    base = 1 << 20                                          # a 256-byte-aligned scratch address
    tau = int(lib.mgs_backward_tau(base, P)) - base
    acc = tau - (P + TAU_SLOTS) * 64
    return dict(P=P, bytes=lib.mgs_backward_bytes(P),
                fields=dict(grad_acc=[acc, P * 64], tau_part=[acc + P * 64, TAU_SLOTS * 64], tau=[tau, 64]))


def main():
    sys.path.insert(0, ROOT)
    from monogs_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("mgs_geometry_bytes", "mgs_image_bytes", "mgs_binning_bytes", "mgs_backward_bytes", "mgs_backward_tau"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    assert lib.mgs_abi_version() == 21, "the recording is the layout of ABI v21"
    out = dict(abi=21,
               geometry=[geometry(lib, P) for P in PS],
               image=[image(lib, W, H) for W, H in WHS],
               binning=[binning(lib, R, W, H) for R in RS for W, H in WHS],
               backward=[backward(lib, P) for P in PS])
    with open(os.path.join(HERE, "scratch_layout.json"), "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": ' + (json.dumps(v) if not isinstance(v, list) else
                                                 "[\n" + ",\n".join(" " + json.dumps(e) for e in v) + "\n]")
                                   for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    main()
