"""The scratch sizes of the feature units (nearest neighbours, mesh sampling, TSDF extraction, stereo) are what the library
returned before their carving functions shared one cursor (csrc/common.h, ScratchCursor): tests/golden/feature_scratch_bytes.json,
made by tests/golden/make_golden_feature_scratch.py from the library of ABI v24.  No GPU needed."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("mgs_knn_scratch_bytes", "mgs_nn_scratch_bytes", "mgs_mesh_sample_scratch_bytes", "mgs_tsdf_extract_scratch_bytes",
             "mgs_stereo_scratch_bytes")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "feature_scratch_bytes.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", FUNCTIONS)
def test_scratch_bytes_are_those_recorded(native_lib, recorded, name):
    fn, rows = getattr(native_lib, name), recorded[name]
    assert recorded["abi"] == 24 and len(rows) >= 3 and set(rows[0]["args"][:-1] or rows[0]["args"]) == {1}
    for row in rows:
        assert fn(*row["args"]) == row["bytes"], (name, row["args"])
