"""The kernels only the mapping window calls -- ``mgs_window_stats``, ``mgs_window_apply``, ``mgs_lr_schedule_step``,
``mgs_sum_buffers`` and ``GaussianAdam`` with its learning rates on the device -- each against a float64 (or exact) PyTorch
statement of the same operation, at the sizes where such kernels break: one element, one short of / one past a wavefront
(64) and a workgroup (256), a prime far past the grid, unaligned buffers, the last visibility word, the grid-stride wrap
(pytest -m gpu).

Every bar below is exact equality, a bound derived from the arithmetic in the comment next to it, or the bar an existing
test of this suite applies to the same quantity (named there)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_LIST = [1, 63, 64, 65, 255, 256, 257, 4097, 100003]
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ---- mgs_window_stats ------------------------------------------------------------------------------------------------
def _stats_inputs(P, K, seed):
    g = _gen(seed)
    grads = [torch.randn(P, 3, generator=g, device=DEV) * (10.0 ** (k % 5 - 4)) for k in range(K)]
    if K >= 2:
        grads[1] = None                                   # a keyframe without a gradient: counted, adds no norm
    if K >= 5:
        grads[K - 1] = None
    radii = [torch.randint(-1, 40, (P,), generator=g, device=DEV, dtype=torch.int32) for _ in range(K)]
    touched = [torch.randint(0, 3, (P,), generator=g, device=DEV, dtype=torch.int32) for _ in range(K)]
    prior = [torch.rand(P, generator=g, device=DEV) * s for s in (1e-2, 7.0, 30.0)]     # non-zero, non-negative contents
    return grads, radii, touched, prior


def _stats_reference(grads, radii, prior, accumulate):
    """The reference's loop over the keyframes (window order): the norm sum in float64; the visible count and the MAX radius
    in float32, one keyframe after the other, which is exact."""
    P = radii[0].shape[0]
    norm = prior[0].double().clone() if accumulate else torch.zeros(P, dtype=torch.float64, device=DEV)
    vis = prior[1].clone() if accumulate else torch.zeros(P, device=DEV)
    maxr = prior[2].clone() if accumulate else torch.zeros(P, device=DEV)
    for g, r in zip(grads, radii):
        v = r > 0
        if g is not None:
            norm += torch.where(v, g[:, :2].double().norm(dim=1), torch.zeros_like(norm))
        vis = torch.where(v, vis + 1.0, vis)
        maxr = torch.where(v, torch.maximum(maxr, r.float()), maxr)
    return norm, vis, maxr


def _packed(touched, words):
    """bit i of word w of row k = (n_touched_k[64 w + i] > 0), zeros beyond P: numpy's little-endian packbits."""
    rows = []
    for t in touched:
        b = np.packbits((t > 0).cpu().numpy(), bitorder="little")
        rows.append(np.concatenate([b, np.zeros(words * 8 - b.shape[0], dtype=np.uint8)]))
    return np.stack(rows)


@pytest.mark.parametrize("K", [1, 2, 5, 30, 32])
@pytest.mark.parametrize("P", P_LIST)
def test_window_stats_matches_the_keyframe_loop(native_lib, P, K):
    from monogs_amd.gaussian_optim import window_stats
    grads, radii, touched, prior = _stats_inputs(P, K, seed=1000 * K + P)
    words = (P + 63) // 64
    worst = 0.0
    for accumulate in (False, True):
        for with_bits in (False, True):
            norm, vis, maxr = (t.clone() for t in prior)
            bits = torch.full((K + 2, words), SENTINEL, dtype=torch.int64, device=DEV) if with_bits else None   # rows > K
            window_stats(grads, radii, touched, norm, vis, maxr, accumulate, bits)
            want_norm, want_vis, want_maxr = _stats_reference(grads, radii, prior, accumulate)
            tag = (P, K, accumulate, with_bits)
            assert torch.equal(vis, want_vis), tag
            assert torch.equal(maxr, want_maxr), tag
            # float32 sum of K non-negative float32 norms against float64: gx*gx + gy*gy carries two roundings (with or
            # without contraction of the second product into the add), the square root one, every add half an ulp of a
            # running sum that never exceeds the final one: (K + 3) * 2^-23 relative to the result bounds all of it
            err = (norm.double() - want_norm).abs()
            bound = (K + 3) * 2.0 ** -23 * want_norm
            assert bool((err <= bound).all()), (tag, float((err - bound).max()))
            worst = max(worst, float((err / want_norm.clamp_min(1e-300)).max()) / ((K + 3) * 2.0 ** -23))
            if with_bits:
                got = bits.cpu().numpy().view(np.uint8).reshape(K + 2, words * 8)
                assert np.array_equal(got[:K], _packed(touched, words)), tag          # (the tail bits beyond P are zero)
                assert bool((bits[K:] == SENTINEL).all()), tag                        # rows >= K untouched
    print(f"window_stats P={P} K={K}: worst norm error / bound = {worst:.3f}")      # measured: at most 0.23 of the bound


def test_window_stats_refuses_bad_arguments_without_launching(native_lib):
    """33 keyframes and a NULL ``radii[k]`` return the error status; the outputs keep their contents."""
    P = 257
    g = _gen(5)
    grad = torch.randn(P, 3, generator=g, device=DEV)
    radii = torch.randint(1, 40, (P,), generator=g, device=DEV, dtype=torch.int32)
    outs = [torch.full((P,), 3.25, device=DEV) for _ in range(3)]
    bits = torch.full((34, (P + 63) // 64), SENTINEL, dtype=torch.int64, device=DEV)
    arr = lambda ps: (C.c_void_p * len(ps))(*ps)  # noqa: E731
    ptr = lambda t: t.data_ptr()  # noqa: E731

    def call(K, radii_ptrs, with_bits):
        return native_lib.mgs_window_stats(P, K, arr([ptr(grad)] * K), arr(radii_ptrs), arr([ptr(radii)] * K), ptr(outs[0]),
                                           ptr(outs[1]), ptr(outs[2]), 0, ptr(bits) if with_bits else None, None)
    assert call(33, [ptr(radii)] * 33, True) == 1
    assert b"keyframes" in native_lib.mgs_last_error()
    assert call(2, [ptr(radii), None], False) == 1
    assert call(2, [None, ptr(radii)], True) == 1
    assert b"NULL" in native_lib.mgs_last_error()
    assert call(-1, [], False) == 1
    torch.cuda.synchronize()
    assert all(bool((o == 3.25).all()) for o in outs) and bool((bits == SENTINEL).all())
    assert call(32, [ptr(radii)] * 32, True) == 0                                    # the largest window is served
    torch.cuda.synchronize()
    assert bool((outs[1] == 32.0).all())


# ---- mgs_window_apply ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", P_LIST)
def test_window_apply_is_plain_float32_arithmetic(native_lib, P):
    g = _gen(P)
    d = [torch.rand(P, generator=g, device=DEV) * s for s in (1e-2, 8.0, 40.0)]
    d[2][::3] = 0.0
    acc = [torch.rand(P, generator=g, device=DEV) * s for s in (3e-2, 100.0, 30.0)]
    want = (acc[0] + d[0], acc[1] + d[1], torch.maximum(acc[2], d[2]))
    rc = native_lib.mgs_window_apply(P, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), acc[0].data_ptr(),
                                     acc[1].data_ptr(), acc[2].data_ptr(), None)
    assert rc == 0
    for got, ref in zip(acc, want):
        assert torch.equal(got, ref)                   # one add / one max per element: bit-equal


# ---- mgs_lr_schedule_step --------------------------------------------------------------------------------------------
def _schedule_cases():
    from monogs_amd.gaussian_map import REFERENCE_LR_SCHEDULE
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "lr_schedule.npz"))
    cases = []
    for i, (a, b, ds, dm, ms) in enumerate(g["cases"]):
        cases.append((f"golden{i}", dict(lr_init=float(a), lr_final=float(b), lr_delay_steps=int(ds), lr_delay_mult=float(dm),
                                         max_steps=int(ms)), {int(s): float(v) for s, v in zip(g["steps"], g[f"lr_{i}"])}))
    cases.append(("reference", dict(REFERENCE_LR_SCHEDULE), {}))
    return cases, [int(s) for s in g["steps"]]


def _within_one_ulp(got: float, want: float) -> bool:
    w = np.float32(want)
    return abs(np.float64(np.float32(got)) - np.float64(w)) <= np.float64(np.spacing(np.abs(w)))


def test_lr_schedule_step_matches_the_golden_and_expon_lr(native_lib):
    """The device schedule (iteration += 1; lr = schedule(iteration)) against the reference's own outputs
    (tests/golden/lr_schedule.npz) and the host's ``expon_lr``: double arithmetic rounded to float32 once, so within one
    float32 ulp of either; the counter advances by exactly one per call."""
    from monogs_amd.gaussian_optim import expon_lr
    cases, golden_steps = _schedule_cases()
    it = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr = torch.full((3,), -7.0, device=DEV)

    def step(s):
        return native_lib.mgs_lr_schedule_step(it.data_ptr(), lr[1:].data_ptr(), s["lr_init"], s["lr_final"],
                                               s["lr_delay_steps"], s["lr_delay_mult"], s["max_steps"], None)
    worst = 0.0
    for name, s, golden in cases:
        # (a) at the golden's step values (the counter preset to step - 1), -1 and 2 000 000 among them
        for want_it in golden_steps:
            it.fill_(want_it - 1)
            assert step(s) == 0
            got = float(lr[1])
            assert int(it) == want_it, (name, want_it)
            want = expon_lr(want_it, **s)
            assert _within_one_ulp(got, want), (name, want_it, got, want)
            if golden:
                assert _within_one_ulp(got, golden[want_it]), (name, want_it, got, golden[want_it])
            if want > 0:
                worst = max(worst, abs(got - want) / float(np.spacing(np.float32(want))))
        # (b) stepped from iteration 0 through max_steps + 5 of a short schedule (the delay, where there is one, ends inside)
        short = dict(s, max_steps=7, lr_delay_steps=min(s["lr_delay_steps"], 3))
        it.zero_()
        for k in range(1, short["max_steps"] + 6):
            assert step(short) == 0
            assert int(it) == k, (name, k)
            want = expon_lr(k, **short)
            assert _within_one_ulp(float(lr[1]), want), (name, k, float(lr[1]), want)
            if short["lr_init"] == 0.0 and short["lr_final"] == 0.0:
                assert float(lr[1]) == 0.0                                   # lr_init = lr_final = 0 gives 0
    assert float(lr[0]) == -7.0 and float(lr[2]) == -7.0                     # one float written, its neighbours untouched
    print(f"lr_schedule: worst |device - expon_lr| = {worst:.2f} float32 ulp")   # measured 0.50 (the rounding to float32)
    # max_steps <= 0 is refused: nothing launched, counter and rate untouched
    it.fill_(41)
    lr.fill_(-7.0)
    for bad in (0, -5):
        assert step(dict(cases[0][1], max_steps=bad)) == 1
        assert b"mgs_lr_schedule_step" in native_lib.mgs_last_error()
    assert int(it) == 41 and bool((lr == -7.0).all())


# ---- mgs_sum_buffers -------------------------------------------------------------------------------------------------
def _carve(count, offset, g, fill=None):
    """A ``count``-float buffer ``offset`` floats into a fresh allocation (allocations are 512-byte aligned: offset 0 is
    16-byte aligned, offset 1 is not), with guard floats on both sides."""
    base = torch.full((count + 8,), 1234.5, device=DEV)
    view = base[offset:offset + count]
    if fill is None:
        view.copy_(torch.randn(count, generator=g, device=DEV))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return base, view


@pytest.mark.parametrize("count", [1, 3, 4, 5, 1023, 2 ** 20 + 3])
@pytest.mark.parametrize("layout", ["aligned", "offset", "mixed", "alias"])
def test_sum_buffers_is_the_left_to_right_float32_sum(native_lib, layout, count):
    """Vector path (all pointers 16-byte aligned) with its scalar tail, scalar path (any pointer unaligned), more than 16
    sources (groups, the running sum first), the result written over the first source: the order of the adds is fixed and
    they are plain float32 adds, so the result is bit-equal to ``((s0 + s1) + s2) + ...``; nothing beyond ``count`` moves."""
    from monogs_amd.gaussian_optim import sum_buffers
    g = _gen(count)
    for n in (1, 2, 15, 16, 17, 31, 32, 37):
        off = {"aligned": lambda k: 0, "alias": lambda k: 0, "offset": lambda k: 1, "mixed": lambda k: k % 2}[layout]
        srcs = [_carve(count, off(k), g) for k in range(n)]
        want = srcs[0][1].clone()
        for _, s in srcs[1:]:
            want = want + s
        if layout == "alias":
            out_base, out = srcs[0]
        else:
            out_base, out = _carve(count, {"aligned": 0, "offset": 1, "mixed": 0}[layout], g, fill=False)
            if layout == "mixed" and n == 1:
                out_base, out = _carve(count, 1, g, fill=False)          # (one source: the unaligned pointer is the output)
        keep = [s.clone() for _, s in srcs]
        got = sum_buffers([s for _, s in srcs], out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out, want), (layout, count, n, float((out - want).abs().max()))
        o = out.storage_offset()
        assert bool((out_base[:o] == 1234.5).all()) and bool((out_base[o + count:] == 1234.5).all()), (layout, count, n)
        for k, ((_, s), s0) in enumerate(zip(srcs, keep)):
            if not (layout == "alias" and k == 0):
                assert torch.equal(s, s0), (layout, count, n, k)          # the sources are read only


# ---- GaussianAdam: learning rates on the device, the grid-stride wrap, skipped tensors, tiny gradients ----------------
WIDTHS = (3, 3, 1, 1, 4)
LRS = (1.6e-4 * 6.0, 0.0025, 0.05, 0.001, 0.001)
OTHER_LRS = (0.004, 0.0007, 0.02, 0.003, 0.0005)


@pytest.mark.parametrize("mode", ["device_lrs", "set_lr_after_device_lrs", "step_10000", "middle_grad_none", "tiny_grads"])
@pytest.mark.parametrize("P", [1, 255, 257, 100003])
def test_gaussian_adam_device_rates_and_edges(native_lib, P, mode):
    """``GaussianAdam`` against ``torch.optim.Adam`` in float32 after every step and against a float64 Adam at the end.
    P = 100 003: 12 P elements exceed the 4096 x 256 threads of the launch, so the grid-stride loop wraps, and the tensor
    boundaries fall inside workgroups."""
    from monogs_amd.gaussian_optim import GaussianAdam
    g = _gen(17 * P)
    scale = 1e-3 if mode == "tiny_grads" else 1.0
    a = [(torch.randn(P, w, generator=g, device=DEV) * scale).requires_grad_(True) for w in WIDTHS]
    lrs = list(LRS)
    fused = GaussianAdam(a, lrs)
    want_lrs = list(LRS)
    if mode in ("device_lrs", "set_lr_after_device_lrs"):
        fused.device_lrs().copy_(torch.tensor(OTHER_LRS, device=DEV))      # the device values differ from `lrs`: they must win
        want_lrs = list(OTHER_LRS)
        assert fused.lrs == [float(x) for x in LRS]
    if mode == "set_lr_after_device_lrs":
        fused.set_lr(0, 0.0123)
        fused.set_lr(4, 0.0042)
        want_lrs[0], want_lrs[4] = 0.0123, 0.0042
        assert fused.lrs[0] == 0.0123 and abs(float(fused.lr_dev[0]) - 0.0123) < 1e-9
    if mode == "tiny_grads":
        # g = 1e-20: g * g underflows, eps = 1e-15 rules the denominator and the update is lr * 1e-5 per step; rates of 1
        # and parameters of 1e-3 keep that update (1e-5 per step, 1.2e-4 in all) far above the absolute bar
        want_lrs = [1.0] * 5
        fused.lrs = [1.0] * 5
    t0 = 10000 if mode == "step_10000" else 0
    fused.t_dev.fill_(t0)

    def reference(dtype):
        ps = [torch.nn.Parameter(t.detach().to(dtype).clone()) for t in a]
        opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(ps, want_lrs)], lr=0.0, eps=1e-15)
        if t0:
            for p in ps:
                opt.state[p] = dict(step=torch.tensor(float(t0)), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
        return ps, opt
    b, ref = reference(torch.float32)
    c, ref64 = reference(torch.float64)
    steps, worst = 12, [0.0, 0.0]
    start = [t.detach().clone() for t in a]
    signs = [1 - 2 * (torch.rand(t.shape, generator=g, device=DEV) < 0.5).float() for t in a]
    for it in range(steps):
        for i, (pa, pb, pc) in enumerate(zip(a, b, c)):
            if mode == "middle_grad_none" and i == 2 and it >= 3:
                pa.grad = pb.grad = pc.grad = None                          # skipped: no step, the count stays
                continue
            if mode == "tiny_grads":
                gr = 1e-20 * signs[i]                                        # (a fixed sign per element: every step moves it on)
            else:
                gr = torch.randn(pa.shape, generator=g, device=DEV) * (10.0 ** (-it / 4))
            pa.grad, pb.grad, pc.grad = gr.clone(), gr.clone(), gr.double()
        fused.step()
        ref.step()
        ref64.step()
        for i, (pa, pb) in enumerate(zip(a, b)):
            tag = (mode, P, it, i)
            st = ref.state[pb]
            # the bars of test_gaussian_adam_matches_torch_adam (parameters) and test_adam_state_surgery_matches_torch (moments)
            assert torch.allclose(pa, pb, rtol=1e-5, atol=3e-6), (tag, float((pa - pb).abs().max()))
            assert torch.allclose(fused.exp_avg[i], st["exp_avg"], rtol=1e-5, atol=1e-7), tag
            assert torch.allclose(fused.exp_avg_sq[i], st["exp_avg_sq"], rtol=1e-5, atol=1e-9), tag
            assert int(fused.t_dev[i]) == int(st["step"]), tag
            worst[0] = max(worst[0], float(((pa - pb).abs() / (1e-5 * pb.abs() + 3e-6)).max().detach()))
    for i, (pa, pc) in enumerate(zip(a, c)):
        assert torch.allclose(pa.double(), pc, rtol=1e-5, atol=3e-6), (mode, P, i, float((pa.double() - pc).abs().max()))
        worst[1] = max(worst[1], float(((pa.double() - pc).abs() / (1e-5 * pc.abs() + 3e-6)).max().detach()))
    skipped = steps - 3 if mode == "middle_grad_none" else 0
    assert fused.t_dev.tolist() == [t0 + steps, t0 + steps, t0 + steps - skipped, t0 + steps, t0 + steps]
    if mode == "tiny_grads":        # the parameters did move by about lr * 1e-5 a step (the check above is not vacuous)
        moved = (a[0].detach() - start[0]).abs()
        assert 0.5e-4 < float(moved.min()) and float(moved.max()) < 2e-4, (float(moved.min()), float(moved.max()))
    print(f"adam {mode} P={P}: worst error / bar = {worst[0]:.3f} (float32 torch), {worst[1]:.3f} (float64)")
    # measured: <= 0.20 of the bar against either reference (step_10000, P = 100 003), <= 0.04 in the other modes
