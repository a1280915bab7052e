"""The per-Gaussian forward kernel now also scans the tiles its workgroup touches (per-tile path) and duplicate_kernel decodes
its slots from 16-byte LDS entries: neither may cost registers that spill or a wave of occupancy.  The compiler's resource
report for gfx950 (no GPU needed) holds every preprocess_forward_kernel and duplicate_kernel instantiation to no scratch
and to the occupancy the same report gave for the commit before the scan was folded in: 8 waves per SIMD for all four
preprocess_forward_kernel<COV, PRECOMP> (40-46 VGPRs, 20 480 bytes of LDS: exactly eight workgroups per compute unit, which is
why the scan keeps its wave totals in the padding of the record hand-over rows) and 8 for duplicate_kernel (51 VGPRs,
9 216 bytes of LDS)."""
import pytest

from resource_report import resource_report

PARENT_OCCUPANCY = 8          # every instantiation of both kernels, parent commit
PARENT_PRE_LDS = 20480        # preprocess_forward_kernel
PARENT_DUP_LDS = 9216         # duplicate_kernel


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    d = tmp_path_factory.mktemp("pre_scan_resources")
    return dict(pre=resource_report("preprocess.hip", d)[0], bin=resource_report("binning.hip", d)[0])


def test_preprocess_forward_keeps_its_occupancy(reports):
    pre = {k: v for k, v in reports["pre"].items() if "preprocess_forward_kernel" in k}
    assert len(pre) == 8, sorted(reports["pre"])          # <COV, PRECOMP> x <SCAN>
    for name, res in pre.items():
        assert int(res["ScratchSize [bytes/lane]"]) == 0, (name, res)
        assert int(res["Occupancy [waves/SIMD]"]) >= PARENT_OCCUPANCY, (name, res)
        assert int(res["LDS Size [bytes/block]"]) <= PARENT_PRE_LDS, (name, res)


def test_duplicate_keeps_its_occupancy(reports):
    dup = {k: v for k, v in reports["bin"].items() if "duplicate_kernel" in k}
    assert len(dup) == 1, sorted(reports["bin"])
    for name, res in dup.items():
        assert int(res["ScratchSize [bytes/lane]"]) == 0, (name, res)
        assert int(res["Occupancy [waves/SIMD]"]) >= PARENT_OCCUPANCY, (name, res)
        assert int(res["LDS Size [bytes/block]"]) <= PARENT_DUP_LDS, (name, res)         # the issue: no larger than before
