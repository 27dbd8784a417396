"""The decode attention bound (tests/decode_ref.py) checked on the CPU: an fp32 emulation of attn_decode_kernel
stays inside it, the flat inputs give bit equality, and the emulation with a planted bug leaves it, which is
the evidence that tests/test_gpu_decode.py would fail for that bug."""
import math

import pytest
import torch

import decode_ref as R

GRID_N = [1, 2, 4, 5, 255, 256, 257, 300, 1024, 4096]


def _case(kind, hs, n, ns, seed):
    B, H, t, scale = 2, 2, n - 1, hs ** -0.5
    if kind == "random":
        return R.build_random(B, H, n, hs, ns, seed), t, scale
    return R.build_needle(B, H, n, hs, ns, t, scale, seed)[:3], t, scale


@pytest.mark.parametrize("kind", ["random", "needle"])
@pytest.mark.parametrize("hs", [8, 24, 32, 64])
def test_fp32_emulation_stays_within_the_bound(kind, hs):
    worst = (-1.0, ())
    for n in GRID_N:
        for ns in (1, 3):
            (q, ks, vs), t, scale = _case(kind, hs, n, ns, seed=1000 * hs + n + ns)
            ref, A = R.decode_attention_ref(q, ks, vs, t, scale)
            r, at = R.worst_ratio(R.emulate_kernel(q, ks, vs, t, scale), ref, A, n)
            worst = max(worst, (r, (n, ns, at)))
    print(f"decode bound, emulation, {kind} hs {hs}: max ratio {worst[0]:.3f} at (n, streams, (b, h, d)) = {worst[1]}")
    assert worst[0] <= 1.0, worst


@pytest.mark.parametrize("shift", [60.0, 100.0])
def test_fp32_emulation_shifted_scores_within_the_bound(shift):
    worst = 0.0
    for hs in (32, 64):
        for t in (63, 5):
            for ns in (1, 2):
                scale = hs ** -0.5
                q, ks, vs = R.build_shifted(2, 2, 64, hs, ns, scale, seed=hs + t + ns, shift=shift)
                sc = scale * torch.einsum("bhd,bhsd->bhs", q.double(), ks[0][:, :, :t + 1].double())
                assert (sc[0, 0] > shift - 8).all() and (sc[0, 1] < -shift + 8).all()  # where the builder says
                ref, A = R.decode_attention_ref(q, ks, vs, t, scale)
                worst = max(worst, R.worst_ratio(R.emulate_kernel(q, ks, vs, t, scale), ref, A, t + 1)[0])
    print(f"decode bound, emulation, shifted {shift:g}: max ratio {worst:.3f}")
    assert worst <= 1.0


def test_missing_max_subtraction_is_seen_at_shift_100_only():
    """exp(+-60) is finite and normal in fp32, so the shift of 60 cannot show a missing max subtraction;
    100 can (inf / inf and 0 / 0). The GPU test runs both."""
    hs, t, scale = 32, 63, 32 ** -0.5
    for shift, seen in ((60.0, False), (100.0, True)):
        q, ks, vs = R.build_shifted(2, 2, 64, hs, 1, scale, seed=3, shift=shift)
        ref, A = R.decode_attention_ref(q, ks, vs, t, scale)
        out = R.emulate_kernel(q, ks, vs, t, scale, no_max=True)
        per_bh = [R.worst_ratio(out[b:b + 1, h:h + 1], ref[b:b + 1, h:h + 1], A[b:b + 1, h:h + 1], t + 1)[0]
                  for b in range(2) for h in range(2)]
        assert all(r > 1.0 for r in per_bh) == seen, (shift, per_bh)


@pytest.mark.parametrize("n", [1, 2, 4, 256, 512, 1024, 4096])
def test_flat_inputs_are_bit_exact_in_the_emulation(n):
    for hs, ns in ((8, 1), (32, 3), (64, 1)):
        q, ks, vs = R.build_flat(2, 2, n + 1, hs, ns, seed=n + hs)
        want = R.flat_expected(vs, n - 1)
        got = R.emulate_kernel(q, ks, vs, n - 1, hs ** -0.5)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (n, hs, ns)
        for extra, drop in ((1, None), (0, torch.full((2, 2, ns), n - 1))):  # a miscount by one is not
            if n == 1 and drop is not None:
                continue  # an empty window has no mean
            bad = R.emulate_kernel(q, ks, vs, n - 1, hs ** -0.5, extra=extra, drop=drop)
            assert not torch.equal(bad.view(torch.int16), want.view(torch.int16)), (n, hs, ns, extra)


def _ratio_per_bh(out, ref, A, n):
    B, H, _ = ref.shape
    r = torch.zeros(B, H)
    for b in range(B):
        for h in range(H):
            r[b, h] = R.worst_ratio(out[b:b + 1, h:h + 1], ref[b:b + 1, h:h + 1], A[b:b + 1, h:h + 1], n)[0]
    return r


@pytest.mark.parametrize("hs", [8, 32, 64])
@pytest.mark.parametrize("n", [300, 4096])
def test_power_planted_bugs_leave_the_bound(n, hs):
    """Needle inputs, 2 x 2 heads x 3 streams (twelve needles over the seven candidate rows). Each planted bug
    must put at least one element of every affected (b, h) outside tol."""
    B, H, ns, t, scale = 2, 2, 3, n - 1, hs ** -0.5
    q, ks, vs, pos = R.build_needle(B, H, n + 1, hs, ns, t, scale, seed=n + hs)
    ref, A = R.decode_attention_ref(q, ks, vs, t, scale)
    assert R.worst_ratio(R.emulate_kernel(q, ks, vs, t, scale), ref, A, n)[0] <= 1.0
    cand = R.needle_candidates(t)
    assert len(set(cand)) == 7 and set(pos.flatten().tolist()) == set(cand)  # every candidate row holds a needle
    # one key dropped: each candidate row in turn (the last key, the last group of four, either side of 256, ...)
    for c in cand:
        drop = torch.where(pos == c, pos, torch.full_like(pos, -1))
        hit = (pos == c).any(dim=-1)
        r = _ratio_per_bh(R.emulate_kernel(q, ks, vs, t, scale, drop=drop), ref, A, n)
        assert hit.any() and (r[hit] > 1.0).all(), (c, r)
        assert (r[~hit] <= 1.0).all(), (c, r)  # and nothing else moved
    # window one row too long: every (b, h) reads its finite stale row t + 1
    r = _ratio_per_bh(R.emulate_kernel(q, ks, vs, t, scale, extra=1), ref, A, n)
    assert (r > 1.0).all(), r
    # streams' V swapped
    r = _ratio_per_bh(R.emulate_kernel(q, ks, vs, t, scale, swap_v=True), ref, A, n)
    assert (r > 1.0).all(), r


def test_a_random_stale_row_is_below_any_bound():
    """Why the GPU tests fill the rows above t with NaN instead of relying on tol: next to a needle a random
    stale row moves the output by about e^-12, far below the output's own bf16 rounding."""
    n, hs = 300, 32
    q, ks, vs, _ = R.build_needle(1, 2, n + 1, hs, 1, n - 1, hs ** -0.5, seed=5)
    g = torch.Generator().manual_seed(6)
    ks[0][:, :, n] = torch.randn(1, 2, hs, generator=g).to(torch.bfloat16)
    vs[0][:, :, n] = torch.randn(1, 2, hs, generator=g).to(torch.bfloat16)
    ref, A = R.decode_attention_ref(q, ks, vs, n - 1, hs ** -0.5)
    assert R.worst_ratio(R.emulate_kernel(q, ks, vs, n - 1, hs ** -0.5, extra=1), ref, A, n)[0] <= 1.0


def test_entry_is_exported_and_refuses_on_the_host():
    """mmt_op_attention_decode validates before any launch, so its refusals need no device."""
    import ctypes

    import mmt_lib as ML
    assert "mmt_op_attention_decode" in ML.EXPORTED
    L = ML.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    arr = (ctypes.c_void_p * 9)(*[p.value] * 9)

    def call(B=2, t=5, T=16, H=2, hs=8, ns=1, q=p, q_ld=48, k=arr, v=arr, kv_ld=48, kv_hs=8, o=p):
        return L.mmt_op_attention_decode(None, B, t, T, H, hs, ns, q, q_ld, k, v, kv_ld, kv_hs, o, 24)

    assert call(hs=12) == -2 and call(hs=0) == -2 and call(hs=128) == -2  # MMT_ERR_UNSUPPORTED
    for kw in (dict(t=16), dict(t=-1), dict(ns=0), dict(ns=9), dict(kv_ld=52), dict(q_ld=52), dict(kv_hs=12),
               dict(B=0), dict(H=0), dict(q=None), dict(o=None), dict(k=None), dict(v=None),
               dict(k=(ctypes.c_void_p * 9)())):
        assert call(**kw) == -1, kw  # MMT_ERR_INVALID


def test_worst_ratio_flags_nan_and_inf():
    ref, A = torch.ones(1, 1, 8, dtype=torch.float64), torch.ones(1, 1, 8, dtype=torch.float64)
    out = torch.ones(1, 1, 8, dtype=torch.bfloat16)
    assert R.worst_ratio(out, ref, A, 4)[0] == 0.0
    out[0, 0, 5] = math.nan
    assert R.worst_ratio(out, ref, A, 4) == (math.inf, (0, 0, 5))
