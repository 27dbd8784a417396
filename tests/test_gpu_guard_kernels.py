"""Kernel-level checks of the guarded optimizer step (include/mmt.h: mmt_grad_sqsum, mmt_guard_finalize,
mmt_adamw_step_guarded) on synthetic tensors: the norm's accuracy and bit-reproducibility, edge inputs,
the non-finite skip, equality with the plain step when nothing clips, the clipped step against an fp64
restatement of the formulas, and the absence of host syncs in `mmt_optim.AdamW.step()`.

Sizes are the smallest at which the kernels take another path: 1 / 3 (tail only), 4 (one vector, no tail),
5 (vector + tail), 255 / 1024 / 1025 (one block's worth and one past it), WRAP_N (two passes of the fixed
grid plus a tail: grad_sqsum_kernel's first two of four unrolled loads are live, the other two masked, and
the loop body runs once; adamw_guarded_kernel's grid-stride loop wraps) and LOOP_N (past two whole
iterations of grad_sqsum_kernel's four-load loop, so the loop carries its accumulators into a second and a
partial third iteration with every unroll slot live, plus a tail: the path every production-size call takes).
"""
import functools
import math

import numpy as np
import pytest
import torch

import mmt_lib as ML
import mmt_optim

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01
GRID = ML.GUARD_SLOTS
WRAP_N = 4 * 256 * GRID * 2 + 7
GUARD_U = 4  # 16-byte loads in flight per thread of grad_sqsum_kernel (csrc/mmt_elem.hip)
LOOP_N = 4 * 256 * GRID * GUARD_U * 2 + 4 * 256 * GRID + 7  # 9 437 191 floats
ULP = 2.0 ** -23  # an fp32 ulp relative to the value (upper bound)
NORM_BOUND = 2.4e-7  # 2 fp32 ulps: the fp64 accumulation error n * 2^-53 is far below one


def _stream():
    return ML.stream_ptr(torch.device("cuda"))


def _new_guard():
    return torch.zeros(ML.lib().mmt_guard_state_bytes(), dtype=torch.uint8, device="cuda")


def _header(guard):
    torch.cuda.synchronize()
    return ML.MmtGuardHeader.from_buffer_copy(guard[:64].cpu().numpy().tobytes())


def _sqsum(g, guard, add=0):
    rc = ML.lib().mmt_grad_sqsum(_stream(), ML.ptr(g), g.numel(), add, ML.ptr(guard))
    assert rc == 0, rc


def _finalize(guard, max_norm=0.0, skip=False):
    rc = ML.lib().mmt_guard_finalize(_stream(), max_norm, 1 if skip else 0, B1, B2, ML.ptr(guard))
    assert rc == 0, rc


def _guarded_step(p, g, m, v, guard, max_norm=0.0, skip=False):
    _sqsum(g, guard)
    _finalize(guard, max_norm, skip)
    rc = ML.lib().mmt_adamw_step_guarded(None, _stream(), ML.ptr(p), ML.ptr(g), ML.ptr(m), ML.ptr(v), p.numel(), LR, B1,
                                         B2, EPS, WD, ML.ptr(guard))
    assert rc == 0, rc


def _plain_step(p, g, m, v, step):
    rc = ML.lib().mmt_adamw_step(None, _stream(), ML.ptr(p), ML.ptr(g), ML.ptr(m), ML.ptr(v), p.numel(), step, LR, B1, B2,
                                 EPS, WD)
    assert rc == 0, rc


@functools.lru_cache(maxsize=None)
def _randn(n, seed=0, std=1.0):
    """A CPU fp32 vector, made once per (n, seed, std) and never modified."""
    return torch.randn(n, generator=torch.Generator().manual_seed(seed + n)) * std


def _ref_norm(*parts):
    return math.sqrt(sum(float((t.double() ** 2).sum()) for t in parts))


# ------------------------------------------------------------------------------------------------ norm
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1024, 1025, WRAP_N, LOOP_N])
def test_norm_matches_fp64_reference(n):
    g = _randn(n)
    guard = _new_guard()
    _sqsum(g.cuda(), guard)
    _finalize(guard)
    h = _header(guard)
    ref = _ref_norm(g)
    err = abs(h.norm - ref) / ref
    print(f"n={n}: norm {h.norm!r} ref {ref!r} rel err {err:.3e}")
    assert err <= NORM_BOUND, (n, h.norm, ref)
    assert h.coef == 1.0 and h.ok == 1 and h.applied_steps == 1


def test_norm_over_three_tensors_equals_norm_of_concatenation():
    parts = [_randn(5, 1), _randn(1024, 2), _randn(70001, 3)]
    guard = _new_guard()
    dev = [t.cuda() for t in parts]
    for k, t in enumerate(dev):
        _sqsum(t, guard, add=1 if k else 0)
    _finalize(guard)
    h = _header(guard)
    ref = _ref_norm(*parts)
    assert abs(h.norm - ref) / ref <= NORM_BOUND, (h.norm, ref)
    one = _new_guard()
    _sqsum(torch.cat(dev), one)
    _finalize(one)
    assert abs(_header(one).norm - ref) / ref <= NORM_BOUND


def test_add_zero_overwrites_stale_slots():
    guard = _new_guard()
    _sqsum(_randn(70001, 3).cuda() * 1e3, guard)  # leaves large partials in many slots
    g = _randn(5, 1)
    _sqsum(g.cuda(), guard, add=0)
    _finalize(guard)
    ref = _ref_norm(g)
    assert abs(_header(guard).norm - ref) / ref <= NORM_BOUND


def test_two_runs_give_byte_identical_state():
    parts = [_randn(5, 1).cuda(), _randn(1024, 2).cuda(), _randn(WRAP_N).cuda(), _randn(LOOP_N).cuda()]
    states = []
    for _ in range(2):
        guard = _new_guard()
        for k, t in enumerate(parts):
            _sqsum(t, guard, add=1 if k else 0)
        _finalize(guard, max_norm=1.0)
        torch.cuda.synchronize()
        states.append(guard.cpu())
    assert torch.equal(states[0][:64], states[1][:64])  # the header
    assert torch.equal(states[0], states[1])  # and every block partial


# ------------------------------------------------------------------------------------------------ edge inputs
def test_all_zeros():
    guard = _new_guard()
    _sqsum(torch.zeros(1025, device="cuda"), guard)
    _finalize(guard, max_norm=1.0, skip=True)
    h = _header(guard)
    assert h.norm == 0.0 and h.coef == 1.0 and h.ok == 1 and (h.applied_steps, h.skipped_steps, h.clipped_steps) == (1, 0, 0)


def test_large_values_do_not_overflow_the_sum():
    """1e20 squared overflows fp32 (1e40) but not fp64: a finite norm, no skip."""
    n = 1025
    guard = _new_guard()
    _sqsum(torch.full((n,), 1e20, device="cuda"), guard)
    _finalize(guard, max_norm=1.0, skip=True)
    h = _header(guard)
    ref = float(np.float32(1e20)) * math.sqrt(n)
    assert math.isfinite(h.norm) and abs(h.norm - ref) / ref <= NORM_BOUND
    assert h.ok == 1 and h.skipped_steps == 0 and h.applied_steps == 1 and h.clipped_steps == 1
    assert 0.0 < h.coef < 1e-20


def test_empty_tensor():
    guard = _new_guard()
    _sqsum(_randn(1025).cuda(), guard)
    _sqsum(torch.zeros(0, device="cuda"), guard, add=1)  # adds nothing
    _finalize(guard)
    ref = _ref_norm(_randn(1025))
    assert abs(_header(guard).norm - ref) / ref <= NORM_BOUND
    _sqsum(torch.zeros(0, device="cuda"), guard, add=0)  # overwrites: an empty gradient has norm 0
    _finalize(guard)
    assert _header(guard).norm == 0.0


NONFINITE = [("nan_in_tail", 1027, 1026, float("nan")), ("inf_in_body", 1027, 17, float("inf"))]


@pytest.mark.parametrize("name,n,pos,val", NONFINITE)
def test_nonfinite_is_skipped_when_asked(name, n, pos, val):
    assert (pos >= n // 4 * 4) == (name == "nan_in_tail")  # the scalar tail / the 16-byte loads
    g = _randn(n).clone()
    g[pos] = val
    guard = _new_guard()
    _sqsum(g.cuda(), guard)
    _finalize(guard, max_norm=1.0, skip=True)
    h = _header(guard)
    assert h.ok == 0 and (h.applied_steps, h.skipped_steps, h.clipped_steps) == (0, 1, 0)
    assert not math.isfinite(h.norm)


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("name,n,pos,val", NONFINITE)
def test_nonfinite_propagates_as_in_torch_without_skip(name, n, pos, val, clip):
    """Without skip_nonfinite the step applies. Reference: torch.nn.utils.clip_grad_norm_ (a NaN norm makes
    every gradient NaN; an infinite one scales by 0, and inf * 0 = NaN) followed by the plain step."""
    g = _randn(n).clone()
    g[pos] = val
    p0 = _randn(n, 7, 0.02)
    pa, ma, va = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    guard = _new_guard()
    _guarded_step(pa, g.cuda(), ma, va, guard, max_norm=clip or 0.0)
    h = _header(guard)
    assert h.ok == 1 and h.applied_steps == 1 and h.skipped_steps == 0
    pb, mb, vb = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    holder = torch.nn.Parameter(torch.zeros(n, device="cuda"))
    holder.grad = g.cuda()
    if clip is not None:
        torch.nn.utils.clip_grad_norm_([holder], clip)
    _plain_step(pb, holder.grad, mb, vb, 1)
    torch.cuda.synchronize()
    for a, b in ((pa, pb), (ma, mb), (va, vb)):
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
    assert torch.isnan(pa).any()
    if clip is not None and name == "nan_in_tail":
        assert torch.isnan(pa).all()


def test_misaligned_pointers_are_refused():
    L = ML.lib()
    buf = torch.zeros(1028, device="cuda")
    odd = buf[1:1025]  # 4 bytes past a 16-byte boundary
    ok = buf[4:1028]
    assert odd.data_ptr() % 16 == 4 and ok.data_ptr() % 16 == 0
    guard = _new_guard()
    INVALID = -1
    assert L.mmt_grad_sqsum(_stream(), ML.ptr(odd), 1024, 0, ML.ptr(guard)) == INVALID
    assert L.mmt_grad_sqsum(_stream(), ML.ptr(ok), -1, 0, ML.ptr(guard)) == INVALID
    assert L.mmt_grad_sqsum(_stream(), ML.ptr(ok), 1024, 0, None) == INVALID
    assert L.mmt_guard_finalize(_stream(), 1.0, 0, B1, B2, None) == INVALID
    for k in range(4):
        t = [ok, ok, ok, ok]
        t[k] = odd
        assert L.mmt_adamw_step_guarded(None, _stream(), *[ML.ptr(x) for x in t], 1024, LR, B1, B2, EPS, WD,
                                        ML.ptr(guard)) == INVALID, k
    assert L.mmt_adamw_step_guarded(None, _stream(), *[ML.ptr(ok)] * 4, 1024, LR, B1, B2, EPS, WD, None) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(guard.cpu(), torch.zeros_like(guard).cpu())  # nothing was launched


# ------------------------------------------------------------------------------------------------ skip
def _opt_run(grads, n, **kw):
    """mmt_optim.AdamW over one parameter of n elements, one step per gradient; returns (p, m, v) after each."""
    p = torch.nn.Parameter(_randn(n, 7, 0.02).cuda())
    opt = mmt_optim.AdamW([p], lr=LR, **kw)
    out = []
    for g in grads:
        p.grad = g.cuda()
        opt.step()
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return opt, out


def test_skipped_step_changes_nothing_and_does_not_advance_the_bias_correction():
    n = 1027
    clean1, clean2 = _randn(n, 11, 1e-3), _randn(n, 12, 1e-3)
    bad = clean1.clone()
    bad[n - 1] = float("nan")
    # a skipped first step: p, m, v as before it, counters (0, 1, 0)
    opt, out = _opt_run([bad], n, skip_nonfinite=True, max_grad_norm=1.0)
    p, m, v = out[0]
    assert torch.equal(p.cpu(), _randn(n, 7, 0.02))
    assert torch.equal(m, torch.zeros_like(m)) and torch.equal(v, torch.zeros_like(v))
    assert opt.counters() == (0, 1, 0)
    assert opt.state_dict()["state"][0]["step"] == 0
    live = opt.state[opt.param_groups[0]["params"][0]]["step"]
    assert torch.is_tensor(live) and live.is_cuda  # state_dict() materialised a copy, the live state keeps the device view
    # the next clean step == step 1 of a fresh guarded optimizer on the same data, bit for bit
    opt_a, out_a = _opt_run([bad, clean1], n, skip_nonfinite=True, max_grad_norm=1.0)
    opt_b, out_b = _opt_run([clean1], n, skip_nonfinite=True, max_grad_norm=1.0)
    for a, b in zip(out_a[1], out_b[0]):
        assert torch.equal(a, b)
    assert opt_a.counters() == (1, 1, 0) and opt_b.counters() == (1, 0, 0)
    # and in the middle of a run: moments and parameters stay, the count does not move
    opt_c, out_c = _opt_run([clean1, bad, clean2], n, skip_nonfinite=True)
    opt_d, out_d = _opt_run([clean1, clean2], n, skip_nonfinite=True)
    for a, b in zip(out_c[1], out_c[0]):
        assert torch.equal(a, b)
    for a, b in zip(out_c[2], out_d[1]):
        assert torch.equal(a, b)
    assert opt_c.counters() == (2, 1, 0) and opt_d.counters() == (2, 0, 0)
    assert float(opt_d.last_grad_norm) == pytest.approx(_ref_norm(clean2), rel=NORM_BOUND)


# ------------------------------------------------------------------------------------------------ against the plain step
def _ulp_distance(a, b):
    """Largest distance in fp32 representation steps (both finite, same sign or zero)."""
    ia, ib = a.view(torch.int32).long(), b.view(torch.int32).long()
    return int((ia - ib).abs().max())


def test_unclipped_guarded_steps_equal_the_plain_step():
    """8 steps from zero moments, no clipping, no skip, against mmt_adamw_step on the same gradients.
    g * 1.0f is exact and both sides compute the bias corrections in fp64 and round once, so bitwise equality
    is expected; the assertion allows one fp32 ulp per element for the single case where the device's fp64
    pow rounds a correction differently from the host's.
    Observed on MI355X: bitwise equal over all 8 steps (the device's and the host's bias corrections were
    identical at every step)."""
    n = 70001
    p0 = _randn(n, 7, 0.02)
    grads = [_randn(n, 20 + k, 1e-3).cuda() for k in range(8)]
    pa, ma, va = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pb, mb, vb = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    guard = _new_guard()
    worst = 0
    for k, g in enumerate(grads):
        _guarded_step(pa, g, ma, va, guard)
        _plain_step(pb, g, mb, vb, k + 1)
        h = _header(guard)
        assert h.coef == 1.0 and h.ok == 1 and h.applied_steps == k + 1
        bc1, bc2s = np.float32(1.0 - float(np.float32(B1)) ** (k + 1)), np.float32(math.sqrt(1.0 - float(np.float32(B2)) ** (k + 1)))
        d = max(_ulp_distance(pa, pb), _ulp_distance(ma, mb), _ulp_distance(va, vb))
        print(f"step {k + 1}: max ulp distance {d}; bias corrections device ({h.bias_correction1!r}, "
              f"{h.bias_correction2_sqrt!r}) host ({float(bc1)!r}, {float(bc2s)!r})")
        worst = max(worst, d)
        assert d <= 1, (k, d)
    print("bitwise equal over 8 steps" if worst == 0 else f"within {worst} ulp over 8 steps")
    h = _header(guard)
    assert (h.applied_steps, h.skipped_steps, h.clipped_steps) == (8, 0, 0)


@pytest.mark.parametrize("fresh", [False, True], ids=["one_gradient", "fresh_gradients"])
def test_clipped_steps_match_fp64_formulas(fresh):
    """Clipping active (max_norm = a quarter of the measured norm), 3 steps from zero moments,
    p ~ N(0, 0.02), g ~ N(0, 1e-3), against the same formulas in fp64 on the CPU from the fp32 inputs.
    one_gradient (one g for all steps: m = (1 - b1^t) g coef has no cancellation, so "ulps of m" is a
    meaningful measure): m and v within 8 fp32 ulps (about four roundings each, 2x margin);
    |p - p_ref| <= 2^-22 |p_ref| + 2^-19 lr per step (an update of at most about lr, about ten roundings).
    fresh_gradients (another g every step, so the recurrences run on changing input under coef < 1):
    b1 m + (1 - b1) g can cancel to near zero, so the error is measured against the magnitude the roundings
    act on, s_m = max_k |g_k coef_k| and s_v = max_k (g_k coef_k)^2 per element (every intermediate of the
    recurrences is bounded by them): |m - m_ref| <= 8 ulp(s_m) t and |v - v_ref| <= 8 ulp(s_v) t after t
    steps: the same four roundings and margin per step, earlier steps' errors carried with weight b < 1."""
    n = 70001
    f32 = lambda x: float(np.float32(x))  # noqa: E731  (the scalars as the C ABI receives them)
    lr, b1, b2, eps, wd = f32(LR), f32(B1), f32(B2), f32(EPS), f32(WD)
    p0 = _randn(n, 7, 0.02)
    grads = [_randn(n, 30 + k, 1e-3) for k in range(3)] if fresh else [_randn(n, 30, 1e-3)] * 3
    c = f32(_ref_norm(grads[0]) / 4)
    p, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pr, mr, vr = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    sm, sv = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    guard = _new_guard()
    for k, g in enumerate(grads):
        _guarded_step(p, g.cuda(), m, v, guard, max_norm=c)
        h = _header(guard)
        norm = _ref_norm(g)
        coef = min(1.0, c / (norm + 1e-6))
        assert coef < 0.3 and h.coef == pytest.approx(coef, rel=4 * ULP) and h.clipped_steps == k + 1
        t = k + 1
        gd = g.double() * coef
        pr = pr * (1.0 - lr * wd)
        mr = mr + (gd - mr) * (1.0 - b1)
        vr = vr * b2 + (1.0 - b2) * gd * gd
        pr = pr - (lr / (1.0 - b1 ** t)) * mr / (vr.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
        sm, sv = torch.maximum(sm, gd.abs()), torch.maximum(sv, gd * gd)
        dm, dv = (m.cpu().double() - mr).abs(), (v.cpu().double() - vr).abs()
        ep = ((p.cpu().double() - pr).abs() / (2.0 ** -22 * pr.abs() + 2.0 ** -19 * lr)).max().item()
        if fresh:
            em, ev = (dm / (ULP * sm)).max().item(), (dv / (ULP * sv)).max().item()
            print(f"step {t}: m {em:.2f} ulps of s_m, v {ev:.3f} ulps of s_v, p {ep:.3f} of its per-step bound")
            assert em <= 8 * t and ev <= 8 * t, (t, em, ev)
        else:
            em, ev = (dm / (ULP * mr.abs())).max().item(), (dv / (ULP * vr.abs())).max().item()
            print(f"step {t}: m {em:.2f} ulps, v {ev:.2f} ulps, p {ep:.3f} of its per-step bound")
            assert em <= 8 and ev <= 8, (t, em, ev)
            assert ep <= t, (t, ep)


# ------------------------------------------------------------------------------------------------ no host sync
def test_guarded_step_does_not_sync():
    n = 70001
    params = [torch.nn.Parameter(_randn(n, 7, 0.02).cuda()), torch.nn.Parameter(_randn(1027, 8, 0.02).cuda())]
    opt = mmt_optim.AdamW(params, lr=LR, max_grad_norm=0.01, skip_nonfinite=True)
    for q in params:
        q.grad = _randn(q.numel(), 40, 1e-3).cuda()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()  # the first step: allocates the guard state and the moments
        opt.step()
        norm = opt.last_grad_norm  # a view, no copy
        with pytest.raises(RuntimeError):  # the mode is live in this build: a real sync raises
            norm.item()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert norm.dim() == 0 and norm.is_cuda
    ref = _ref_norm(_randn(n, 40, 1e-3), _randn(1027, 40, 1e-3))
    assert float(norm) == pytest.approx(ref, rel=NORM_BOUND)
    assert opt.counters() == (2, 0, 2)
