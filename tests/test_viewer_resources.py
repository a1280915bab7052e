"""The viewer kernels (csrc/viewer.hip) compile for gfx950 with the Makefile's flags, without warnings and without scratch: the
ellipsoid walk keeps a pixel's colour, hit and "open" state per lane and fetches a candidate's record with scalar loads, and a
spill there would be a design error.  The register, occupancy and LDS figures are printed; DESIGN.md quotes the walk's.  No GPU."""
from resource_report import resource_report

KERNELS = ("viewer_ellipsoids_kernel", "viewer_empty_kernel", "viewer_lines_kernel", "viewer_max_kernel", "viewer_compose_kernel")


def test_viewer_kernels_do_not_spill(tmp_path):
    report, stderr = resource_report("viewer.hip", tmp_path)
    assert "warning:" not in stderr, stderr[-4000:]
    kernels = report
    for want in KERNELS:
        found = {k: v for k, v in kernels.items() if want in k}
        assert len(found) == 1, (want, sorted(kernels))
        (name, res), = found.items()
        what = (want, "VGPRs", res["VGPRs"], "SGPRs", res["TotalSGPRs"], "waves/SIMD", res["Occupancy [waves/SIMD]"],
                "LDS bytes", res["LDS Size [bytes/block]"])
        print(what)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
        assert int(res["LDS Size [bytes/block]"]) == 0, what
    # what only the viewer kernels and the shared clears live in this file
    assert all(any(w in k for w in KERNELS) or "zero_fill" in k for k in kernels), sorted(kernels)
