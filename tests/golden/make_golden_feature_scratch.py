#!/usr/bin/env python3
"""Writes tests/golden/feature_scratch_bytes.json: what the five `*_scratch_bytes` entry points of the feature units (knn.hip,
mesheval.hip, tsdf.hip, stereo.hip) returned at ABI v24, before their carving functions shared one cursor (csrc/common.h,
ScratchCursor).  tests/test_feature_scratch_bytes.py holds every later library against the file.

Per size argument: 1, a value that is no multiple of the unit's box (64 points), scan block (2048 items) or alignment (256 bytes),
and a value one past a multiple.  Run with a library of ABI v24 from before the change (MGS_LIB_PATH) to regenerate; sizes that are
MEANT to move get a new recording."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

CASES = {
    "mgs_knn_scratch_bytes": [[1], [5000], [6145]],                          # P; boxes of 64
    "mgs_nn_scratch_bytes": [[1, 1], [5000, 7003], [6145, 8193]],            # Q, P; boxes of 64
    "mgs_mesh_sample_scratch_bytes": [[1], [5000], [4097]],                  # T; scan blocks of 2048
    "mgs_tsdf_extract_scratch_bytes": [[1, 1, 1], [10, 11, 13], [2049, 1, 1]],     # nx, ny, nz; scan blocks of 2048 voxels
    "mgs_stereo_scratch_bytes": [[1, 1, 16], [100, 37, 32], [273, 1, 16], [752, 480, 64]],   # W, H, D; 256-byte sub-buffers
}


def main():
    sys.path.insert(0, ROOT)
    from monogs_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    assert lib.mgs_abi_version() == 24, "the recording is the sizes of ABI v24"
    out = {"abi": 24}
    for name, cases in CASES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        out[name] = [{"args": args, "bytes": int(fn(*args))} for args in cases]
    with open(os.path.join(HERE, "feature_scratch_bytes.json"), "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": ' + (json.dumps(v) if not isinstance(v, list) else
                                                 "[\n" + ",\n".join(" " + json.dumps(e) for e in v) + "\n]")
                                   for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    main()
