"""The label kernels (csrc/labels.hip) keep a pixel's K <= 8 or K <= 24 values in registers, four pixels per lane on the 16-byte
route.  The compiler's resource report for gfx950 (no GPU needed) must show no scratch for any kernel of the file: a spilled
instantiation is a wrong choice of chunk, not something to accept.  The register, occupancy and LDS figures are printed; DESIGN.md
section 3 ("Label kernels") quotes them."""
from resource_report import resource_report


def test_label_kernels_do_not_spill(tmp_path):
    report, stderr = resource_report("labels.hip", tmp_path)
    assert "warning:" not in stderr, stderr[-4000:]
    kernels = {k: v for k, v in report.items() if "label_" in k}
    loss = {k: v for k, v in kernels.items() if "label_loss_kernel" in k}
    count = {k: v for k, v in kernels.items() if "label_count_kernel" in k}
    conf = {k: v for k, v in kernels.items() if "label_confusion_kernel" in k}
    fin = {k: v for k, v in kernels.items() if "finalize_kernel" in k}
    # (16-byte or scalar route) x (K <= 8, K <= 24 in registers, two passes); either route of the count; LDS or global confusion
    assert len(loss) == 6 and len(count) == 2 and len(conf) == 2 and len(fin) == 2, sorted(kernels)
    assert len(kernels) == 12, sorted(kernels)
    for name, res in kernels.items():
        what = (name, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "waves/SIMD", res["Occupancy [waves/SIMD]"],
                "LDS bytes", res["LDS Size [bytes/block]"])
        print(what)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
    # the staged confusion matrix is the only LDS beyond a few words of reduction: 64 x 64 counts
    lds = sorted(int(v["LDS Size [bytes/block]"]) for v in conf.values())
    assert lds[0] <= 64 and 64 * 64 * 4 <= lds[1] <= 64 * 64 * 4 + 64, lds
    # built (VGPRs / waves per SIMD): loss, 16-byte route: K <= 8: 89 / 5, K <= 24: 170 / 2, two passes: 119 / 4; scalar route:
    # 51 / 7, 104 / 4, 46 / 7; count 10 / 8 and 8 / 8; confusion 14 / 8 either way, 16400 bytes of LDS staged.
