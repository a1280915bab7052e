"""Banded tile sort: the kernels it adds or changes keep their place on the chip.  From the compiler's resource report for
gfx950 (no GPU needed): no scratch, LDS within the eight-workgroups-per-CU budget (160 KiB / 8 = 20 480 bytes), and the
band counters did not cost preprocess_forward_kernel any occupancy or any LDS (they live in the padding of its hand-over
rows)."""
import pytest

from resource_report import resource_report

LDS_BUDGET = 20480          # bytes per workgroup: eight workgroups per compute unit


def _kernels(unit, tmp_path, needle):
    kernels = resource_report(unit, tmp_path)[0]
    found = {k: v for k, v in kernels.items() if needle in k}
    assert found, (needle, sorted(kernels))
    return found


def test_preprocess_scan_instantiations_keep_lds_and_occupancy(tmp_path):
    kernels = _kernels("preprocess.hip", tmp_path, "preprocess_forward_kernel")
    assert len(kernels) == 8, sorted(kernels)
    scan = {k: v for k, v in kernels.items() if k.endswith("Lb1EEEvNS_7PreArgsE")}       # <COV, PRECOMP, SCAN = true>
    plain = {k: v for k, v in kernels.items() if k.endswith("Lb0EEEvNS_7PreArgsE")}
    assert len(scan) == 4 and len(plain) == 4, sorted(kernels)
    for name, k in kernels.items():
        assert int(k["ScratchSize [bytes/lane]"]) == 0, (name, k)
        assert int(k["LDS Size [bytes/block]"]) == LDS_BUDGET, (name, k)
    for name, k in scan.items():
        twin = plain[name.replace("Lb1EEEvNS_7PreArgsE", "Lb0EEEvNS_7PreArgsE")]
        assert int(k["Occupancy [waves/SIMD]"]) >= int(twin["Occupancy [waves/SIMD]"]), (name, k, twin)


@pytest.mark.parametrize("needle", ["emit_banded_kernel", "scan_blocks_kernel", "duplicate_kernel"])
def test_binning_kernels_no_scratch_lds_in_budget(tmp_path, needle):
    for name, k in _kernels("binning.hip", tmp_path, needle).items():
        assert int(k["ScratchSize [bytes/lane]"]) == 0, (name, k)
        assert int(k["LDS Size [bytes/block]"]) <= LDS_BUDGET, (name, k)
        if needle == "emit_banded_kernel":       # 256 threads: eight workgroups per CU need eight waves per SIMD
            assert int(k["Occupancy [waves/SIMD]"]) >= 8, (name, k)


def test_radix_pass_and_histogram_kernels_banded_and_plain(tmp_path):
    """radix_sort.hip: the segmented pass and its histogram are the plain kernels' bodies with BANDED set, so both forms are held
    here.  The 3072-pair pass (ITEMS = 12) is the one the flagship sort runs: 72 VGPRs is what lets seven workgroups per CU hold
    every sort tile at once, and the band values it adds must stay in scalar registers (as vector registers they spilled)."""
    kernels = resource_report("radix_sort.hip", tmp_path)[0]
    pick = lambda needle: {k: v for k, v in kernels.items() if needle in k}          # noqa: E731
    banded_pass, banded_hist = pick("rs_pass_banded_kernel"), pick("rs_tile_hist_banded_kernel")
    assert len(banded_pass) == 2 and len(banded_hist) == 4, (sorted(banded_pass), sorted(banded_hist))
    for name, k in {**banded_pass, **banded_hist, **pick("rs_tile_hist_kernel")}.items():
        assert int(k["ScratchSize [bytes/lane]"]) == 0, (name, k)
    (wide,) = [v for k, v in banded_pass.items() if "ILi12EE" in k]
    assert int(wide["VGPRs"]) <= 72 and int(wide["Occupancy [waves/SIMD]"]) >= 7, wide
    assert int(wide["LDS Size [bytes/block]"]) <= LDS_BUDGET, wide
    # the plain pass of the same tile size keeps its place: rs_pass_kernel<12, 8, SCANNED, !PAYLOAD, !BALLOT, !VIDX>
    (plain,) = pick("rs_pass_kernelILi12ELi8ELb1ELb0ELb0ELb0EE").values()
    assert int(plain["VGPRs"]) == 72 and int(plain["ScratchSize [bytes/lane]"]) == 0, plain
    assert int(plain["Occupancy [waves/SIMD]"]) == 7 and int(plain["LDS Size [bytes/block]"]) == 18644, plain
    # one tile per workgroup: the eight-workgroup budget holds.  Four tiles per workgroup (1024 threads) count into 4 x 16 KB
    # of LDS by construction, as rs_tile_hist_kernel<*, 4, *> always has: that budget does not apply, 160 KB / 64 KB = two do
    for name, k in banded_hist.items():
        lds = int(k["LDS Size [bytes/block]"])
        assert lds <= (LDS_BUDGET if name.endswith("ELi1EEEvNS_14RsTileHistArgsE") else 4 * 16384 + 512), (name, k)
