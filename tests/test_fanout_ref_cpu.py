"""The fan-out decode attention bound (tests/fanout_ref.py) checked on the CPU: an fp32 emulation of
attn_decode_fanout_kernel (tiled prefix, running rescale, per-sample tail) stays inside it, flat inputs give bit
equality, and the emulation with a planted bug leaves it on every affected (row, head), which is the evidence that
tests/test_gpu_decode_fanout.py would fail for that bug.

A fan-out window has at least two keys (n0 >= 1 prefix rows and the row of position t >= n0), so the grid starts at
n = 2 where decode_ref's starts at 1."""
import pytest
import torch

import fanout_ref as F

# (n0, t): n = 2 and 3, either side of a 64-key tile boundary in the prefix and in the tail, n = 300 three ways,
# n = 4096 with a short and with a long tail
GRID = [(1, 1), (1, 2), (2, 2), (63, 63), (64, 64), (65, 65), (63, 126), (64, 127), (64, 128), (65, 129), (1, 64),
        (1, 65), (250, 299), (1, 299), (290, 299), (4000, 4095), (64, 4095)]


def _inputs(kind, hs, n0, t, ns, seed):
    B, S, H, scale = 2, 3, 2, hs ** -0.5
    cap = t - n0 + 2
    if kind == "random":
        return F.build_random(B, S, H, n0 + 1, hs, ns, cap, seed), scale
    return F.build_needle(B, S, H, n0 + 1, hs, ns, cap, n0, t, scale, seed)[:5], scale


@pytest.mark.parametrize("kind", ["random", "needle"])
@pytest.mark.parametrize("hs", [8, 24, 32, 64])
def test_fp32_emulation_stays_within_the_bound(kind, hs):
    worst = (-1.0, ())
    for n0, t in GRID:
        for ns in ((1, 3) if t < 1000 else (1,)):
            (q, ks, vs, tks, tvs), scale = _inputs(kind, hs, n0, t, ns, seed=1000 * hs + 7 * n0 + t + ns)
            ref, A = F.fanout_attention_ref(q, ks, vs, tks, tvs, n0, t, scale)
            r, at = F.worst_ratio(F.emulate_kernel(q, ks, vs, tks, tvs, n0, t, scale), ref, A, t + 1, n0)
            worst = max(worst, (r, (n0, t, ns, at)))
    print(f"fan-out bound, emulation, {kind} hs {hs}: max ratio {worst[0]:.3f} at (n0, t, streams, index) = {worst[1]}")
    assert worst[0] <= 1.0, worst


def test_the_extra_term_is_small_next_to_the_base_bound():
    """3 nt 2^-22 A against (n + 256) 2^-22 A: the rescale chain may add at most a few percent."""
    for n0, t in GRID:
        n = t + 1
        assert 3 * F.tiles(n0, n) <= 0.06 * (n + 256), (n0, t)


@pytest.mark.parametrize("shift", [60.0, 100.0])
def test_fp32_emulation_shifted_scores_within_the_bound(shift):
    worst = 0.0
    for hs in (32, 64):
        for n0, t in ((7, 9), (70, 140)):
            scale = hs ** -0.5
            q, ks, vs, tks, tvs = F.build_shifted(2, 4, 2, n0, hs, 2, t - n0 + 1, scale, seed=hs + t, shift=shift)
            sc = scale * torch.einsum("bshd,bhkd->bshk", q.double(), ks[0].double())
            st = scale * torch.einsum("bshd,bshkd->bshk", q.double(), tks[0].double())
            assert (sc[:, 0::2] > shift - 8).all() and (st[:, 0::2] < -shift + 8).all()  # even: prefix high, tail low
            assert (sc[:, 1::2] < -shift + 8).all() and (st[:, 1::2] > shift - 8).all()  # odd: the other way round
            ref, A = F.fanout_attention_ref(q, ks, vs, tks, tvs, n0, t, scale)
            out = F.emulate_kernel(q, ks, vs, tks, tvs, n0, t, scale)
            worst = max(worst, F.worst_ratio(out, ref, A, t + 1, n0)[0])
            if shift == 100.0:  # and a dropped rescale is seen where the maximum moves up: the odd samples
                bad = F.ratio_per_row_head(F.emulate_kernel(q, ks, vs, tks, tvs, n0, t, scale, bug="no_rescale"),
                                           ref, A, t + 1, n0)
                assert (bad[:, 1::2] > 1.0).all(), bad
    print(f"fan-out bound, emulation, shifted {shift:g}: max ratio {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("n0,t", [(1, 1), (2, 3), (48, 63), (64, 127), (200, 255), (1000, 1023), (4000, 4095)])
def test_flat_inputs_are_bit_exact_in_the_emulation(n0, t):
    for hs, ns in ((8, 1), (32, 3), (64, 1)):
        cap = t - n0 + 2
        q, ks, vs, tks, tvs = F.build_flat(2, 3, 2, n0, hs, ns, cap, seed=t + hs)
        want = F.flat_expected(vs, tvs, n0, t)
        got = F.emulate_kernel(q, ks, vs, tks, tvs, n0, t, hs ** -0.5)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (n0, t, hs, ns)
        for bug in ("tail_long",) + (("tail_short",) if t > n0 else ()):  # a miscount by one is not
            bad = F.emulate_kernel(q, ks, vs, tks, tvs, n0, t, hs ** -0.5, bug=bug)
            assert not torch.equal(bad.view(torch.int16), want.view(torch.int16)), (n0, t, hs, ns, bug)


@pytest.mark.parametrize("hs", [8, 32, 64])
@pytest.mark.parametrize("n0,t", [(250, 299), (4000, 4095)])
def test_power_planted_bugs_leave_the_bound(n0, t, hs):
    """Needle inputs, 2 prompts x 4 samples x 2 heads x 2 streams. Each planted bug must put at least one element
    of every affected (row, head) outside the bound."""
    B, S, H, ns, scale = 2, 4, 2, 2, hs ** -0.5
    n, L = t + 1, t - n0 + 1
    q, ks, vs, tks, tvs, pp, tp = F.build_needle(B, S, H, n0 + 1, hs, ns, L + 1, n0, t, scale, seed=n + hs)
    ref, A = F.fanout_attention_ref(q, ks, vs, tks, tvs, n0, t, scale)
    assert F.worst_ratio(F.emulate_kernel(q, ks, vs, tks, tvs, n0, t, scale), ref, A, n, n0)[0] <= 1.0
    assert set(pp.flatten().tolist()) == set(F.prefix_candidates(n0)) >= {0, n0 - 1}
    assert set(tp[:, 1::2].flatten().tolist()) == set(F.tail_candidates(L)) >= {0, L - 1}
    even = torch.zeros(B, S, H, dtype=torch.bool)
    even[:, 0::2] = True
    last_tile = (n0 - 1) // F.KT * F.KT
    affected = {
        "prefix_prompt": even,                                            # their needle sits in the prompt's prefix
        "tail_sample": ~even,                                             # theirs in their own tail
        "tail_long": torch.ones_like(even),                               # the stale row: own key, value negated
        "tail_short": ~even & (tp == L - 1).any(-1),                      # needle in the last tail row
        "no_rescale": ~even | (even & (pp >= F.KT).any(-1)[:, None]),     # the maximum moves after the first tile
        "early_tail": even & (pp >= last_tile).any(-1)[:, None],          # needle in the last prefix tile
    }
    for bug in F.BUGS:
        r = F.ratio_per_row_head(F.emulate_kernel(q, ks, vs, tks, tvs, n0, t, scale, bug=bug), ref, A, n, n0)
        hit = affected[bug]
        assert hit.any() and (r[hit] > 1.0).all(), (bug, r)


def test_entry_is_exported_and_refuses_on_the_host():
    """mmt_op_attention_decode_fanout validates before any launch, so its refusals need no device."""
    import ctypes

    import mmt_lib as ML
    assert "mmt_op_attention_decode_fanout" in ML.EXPORTED
    L = ML.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    arr = (ctypes.c_void_p * 9)(*[p.value] * 9)

    def call(B=2, S=3, n0=4, t=5, T=16, H=2, hs=8, ns=1, q=p, q_ld=48, k=arr, v=arr, kv_ld=48, kv_hs=8, tk=arr, tv=arr,
             t_ld=48, t_rows=4, o=p):
        return L.mmt_op_attention_decode_fanout(None, B, S, n0, t, T, H, hs, ns, q, q_ld, k, v, kv_ld, kv_hs, tk, tv,
                                                t_ld, t_rows, o, 24)

    assert call(hs=12) == -2 and call(hs=0) == -2 and call(hs=128) == -2  # MMT_ERR_UNSUPPORTED
    for kw in (dict(t=16), dict(t=-1), dict(ns=0), dict(ns=9), dict(kv_ld=52), dict(q_ld=52), dict(kv_hs=12),
               dict(t_ld=52), dict(B=0), dict(H=0), dict(S=0), dict(S=-1), dict(n0=0), dict(n0=6), dict(t_rows=0),
               dict(t_rows=2, n0=3), dict(q=None), dict(o=None), dict(k=None), dict(v=None), dict(tk=None),
               dict(tv=None), dict(tk=(ctypes.c_void_p * 9)()), dict(k=(ctypes.c_void_p * 9)())):
        assert call(**kw) == -1, kw  # MMT_ERR_INVALID
