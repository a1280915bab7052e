"""The pose-tangent kernels (csrc/pose_tangent.hip) and the Gauss-Newton kernels (csrc/gauss_newton.hip) in the compiler's resource
report for gfx950 (no GPU needed): no kernel spills to scratch -- the tangent blend keeps 30 accumulators per lane and the step
kernel an unrolled 8 x 8 Cholesky in registers, so a spill would be a wrong layout, not something to accept --, the tangent blend
uses no LDS, and neither unit compiles with a warning.  Registers, SGPRs and occupancy are printed; DESIGN.md section 3 ("Pose
tangents") quotes them."""
from resource_report import resource_report

TANGENT = ("pose_tangent_records_kernel", "pose_tangent_blend_kernel")
GAUSS_NEWTON = ("gn_normal_partial_kernel", "gn_normal_reduce_kernel", "pose_gn_step_kernel")


def _check(unit, names, tmp_path):
    report, stderr = resource_report(unit, tmp_path)
    assert "warning:" not in stderr, stderr[-4000:]
    found = {}
    for want in names:
        hit = {k: v for k, v in report.items() if want in k}
        assert len(hit) == 1, (want, sorted(report))
        found.update(hit)
    for name, res in found.items():
        what = (name, "VGPRs", res["VGPRs"], "AGPRs", res.get("AGPRs"), "SGPRs", res["TotalSGPRs"], "waves/SIMD",
                res["Occupancy [waves/SIMD]"], "LDS bytes", res["LDS Size [bytes/block]"])
        print(what)
        assert int(res["ScratchSize [bytes/lane]"]) == 0, what
    return found


def test_pose_tangent_kernels_do_not_spill_and_the_blend_uses_no_lds(tmp_path):
    found = _check("pose_tangent.hip", TANGENT, tmp_path)
    (blend,) = [v for k, v in found.items() if "pose_tangent_blend_kernel" in k]
    assert int(blend["LDS Size [bytes/block]"]) == 0, blend
    assert int(blend["TotalSGPRs"]) <= 102, blend          # a wave's scalar registers: beyond them the records would spill


def test_gauss_newton_kernels_do_not_spill(tmp_path):
    _check("gauss_newton.hip", GAUSS_NEWTON, tmp_path)
