"""duplicate_kernel turns slot t of a rectangle w tiles wide into (t / w, t % w) with a float32 reciprocal multiply and one
correction step instead of a 32-bit integer division (dup_divmod, csrc/binning.hip), where the grid has at most 2^16 tiles.
The formula, restated in numpy float32, is run over EVERY t < 65 536 and 1 <= w <= 4 096 against integer division.

The kernel's reciprocal is v_rcp_f32, good to 1 ulp, with two ulps taken off so that it never exceeds 1 / w.  numpy's
1 / w is correctly rounded, so the check runs with that reciprocal lowered by 1, 2 and 3 ulps: every value the hardware
instruction may return, lowered by two."""
import numpy as np


def _divmod_mirror(t, w, ulps_off):
    """t: uint32 array, w: int.  The kernel's arithmetic, one float32 operation per operator."""
    r = (np.float32(1.0) / np.float32(w)).view(np.uint32) - np.uint32(ulps_off)
    r = r.view(np.float32)
    q = (t.astype(np.float32) * r).astype(np.uint32)              # float -> uint conversion truncates, as v_cvt_u32_f32
    rem = t - q * np.uint32(w)                                    # (wraps like the kernel's uint32 if q were too large)
    fix = rem >= np.uint32(w)
    return np.where(fix, q + np.uint32(1), q), np.where(fix, rem - np.uint32(w), rem)


def test_reciprocal_divmod_is_exact_on_the_whole_domain():
    t = np.arange(65536, dtype=np.uint32)
    for w in range(1, 4097):
        q_ref, r_ref = t // np.uint32(w), t % np.uint32(w)
        for ulps in (1, 2, 3):
            q, rem = _divmod_mirror(t, w, ulps)
            assert np.array_equal(q, q_ref) and np.array_equal(rem, r_ref), (w, ulps)
