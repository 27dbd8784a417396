"""Host side of generate(num_samples=S, rolling=True), no GPU: the predicate (mmt_rollout.rolls), the schedule
(rolling_step / rolling_schedule), the path generate reports, the arithmetic of mmt_rolling_bytes and the refusals of
mmt_rolling_step that need no device."""
import ctypes

import pytest
import torch

import config_utils
import mmt_lib as ML
import mmt_rollout as MR
import model as mmt_model

M3, V3, CROSS3 = 3, [37, 5, 11], [True, False, False]
T = 24


def _shapes(B, n0, M=3):
    return [(B, n0)] * M


# ------------------------------------------------------------------------------------------------ the predicate
GOOD = dict(cache=True, shapes=_shapes(2, T), N=6, S=3, T=T, rolling=True)


def _rolls(**kw):
    a = dict(GOOD, **kw)
    return MR.rolls(a["cache"], a["shapes"], a["N"], a["S"], a["T"], a["rolling"])


def test_predicate_holds_and_each_condition_flips_it():
    assert _rolls() is True
    flips = {
        "rolling absent": dict(rolling=False),
        "rolling None": dict(rolling=None),
        "no num_samples": dict(S=None),
        "the cache rule": dict(cache=False),
        "a prompt that is not [B, n0]": dict(shapes=[(2, T), (2, T), (2, T, 1)]),
        "prompts of unequal lengths": dict(shapes=[(2, T), (2, T - 1), (2, T)]),
        "an empty prompt": dict(shapes=_shapes(2, 0), N=T),
        "no new token": dict(N=0),
        "N > T": dict(N=T + 1),
        "a prompt longer than the block": dict(shapes=_shapes(2, T + 1)),
        "a call that stays inside the block": dict(shapes=_shapes(2, T - 6)),
        "a call whose last step reads exactly T tokens": dict(shapes=_shapes(2, T - 5)),
    }
    for what, kw in flips.items():
        assert _rolls(**kw) is False, what
    # the edges on the good side: N = T; n0 = 1 with N = T would read at most T tokens, so the smallest prompt that
    # rolls at N = T is n0 = 2; the last step of n0 = T - 4, N = 6 reads T + 1 tokens
    assert _rolls(N=T) is True
    assert _rolls(shapes=_shapes(1, 2), N=T) is True
    assert _rolls(shapes=_shapes(1, 1), N=T) is False
    assert _rolls(shapes=_shapes(2, T - 4)) is True
    assert _rolls(S=1) is True


def test_without_the_keyword_the_path_is_todays():
    """rolling absent: generate_path is fans_out's answer, "fanout" or "tiled", for every input tried; with the
    keyword a call fans_out accepts stays "fanout"."""
    for cache in (True, False):
        for S in (None, 1, 3):
            for n0 in (0, 1, 5, T - 6, T - 5, T, T + 3):
                for N in (0, 1, 6, T, T + 1):
                    for shapes in (_shapes(2, n0), [(2, n0), (2, n0 + 1), (2, n0)], [(2, n0, 1)] * 3):
                        fan = MR.fans_out(cache, shapes, N, S, T)
                        want = "fanout" if fan else "tiled"
                        assert MR.generate_path(cache, shapes, N, S, T) == want
                        assert MR.generate_path(cache, shapes, N, S, T, False) == want
                        got = MR.generate_path(cache, shapes, N, S, T, True)
                        if fan:
                            assert got == "fanout" and not MR.rolls(cache, shapes, N, S, T, True)
                        else:
                            assert got == ("rolling" if MR.rolls(cache, shapes, N, S, T, True) else "tiled")


# ------------------------------------------------------------------------------------------------- the schedule
def _check_schedule(n0, N):
    """Every j: the existing steps while n <= T, then (k, m, p) with p + m == T, m == j, p >= 1, k = n - T, the
    prefix columns k..n0-1 are p long and the tail columns n - m..n - 1 start at n0."""
    sched = MR.rolling_schedule(n0, N, T)
    assert len(sched) == N
    rolled = 0
    for j, step in enumerate(sched):
        n = n0 + j
        assert step == MR.rolling_step(n0, j, T)
        if n <= T:
            assert step is None, (n0, N, j)
            continue
        k, m, p = step
        rolled += 1
        assert p + m == T and m == j and p >= 1 and k == n - T, (n0, N, j, step)
        assert n0 - k == p and n - m == n0
    return sched, rolled


def test_schedule_full_window():
    sched, rolled = _check_schedule(T, 6)
    assert sched[0] is None and rolled == 5  # the prefill over the full window, then every step rolls
    assert sched[1] == (1, 1, T - 1) and sched[5] == (5, 5, T - 5)
    assert MR.rolls(True, _shapes(2, T), 6, 3, T, True)


def test_schedule_mixed():
    """n0 < T < n0 + N: the first T - n0 + 1 steps are the existing ones (the prefill, T - n0 fan-out steps), the
    rest roll."""
    for n0, N in ((T - 2, 6), (T - 1, 3), (5, T), (T - 7, 9)):
        sched, rolled = _check_schedule(n0, N)
        first = T - n0 + 1
        assert all(s is None for s in sched[:first]) and all(s is not None for s in sched[first:])
        assert rolled == N - first and rolled >= 1
        assert MR.rolls(True, _shapes(1, n0), N, 2, T, True)
        assert MR.generate_path(True, _shapes(1, n0), N, 2, T, True) == "rolling"


def test_schedule_longest_call_and_the_refused_one():
    sched, rolled = _check_schedule(T, T)  # N = T: the last step shares one row, p = 1
    assert sched[-1] == (T - 1, T - 1, 1) and rolled == T - 1
    assert MR.generate_path(True, _shapes(2, T), T, 3, T, True) == "rolling"
    # N = T + 1 would need p = 0 at its last step: refused, the call is tiled as without the keyword
    assert MR.rolling_step(T, T, T) == (T, T, 0)
    assert not MR.rolls(True, _shapes(2, T), T + 1, 3, T, True)
    assert MR.generate_path(True, _shapes(2, T), T + 1, 3, T, True) == "tiled"
    assert MR.generate_path(True, _shapes(2, T), T + 1, 3, T) == "tiled"


def test_generate_validates_rolling_before_touching_a_device():
    config_utils._config_cache = {"n_embd": 32, "n_head": 4, "n_layer": 1, "block_size": 8, "dropout": 0.0,
                                  "device": "cpu", "batch_size": 2, "eval_iters": 1}
    m = mmt_model.MultimodalTransformer(2, [11, 5], [[None] * 8 + [c] + [None] * 3 for c in (True, False)])
    m.eval()
    prompts = [torch.zeros(2, 8, dtype=torch.long), torch.zeros(2, 8, dtype=torch.long)]
    with pytest.raises(ValueError, match="num_samples"):  # rolling without num_samples is out of scope
        m.generate(prompts, max_new_tokens=3, rolling=True)
    with pytest.raises(RuntimeError, match="ROCm GPU"):  # a CPU-resident model has no path, as before
        m.generate(prompts, max_new_tokens=3, num_samples=2, rolling=True)
    assert m.last_generate_path == "tiled"
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.generate(prompts, max_new_tokens=3, modality_to_generate=[0], num_samples=2, rolling=True)


# ------------------------------------------------------------------------------------- the C entries on the host
def _rup(x, a=256):
    return -(-x // a) * a


def _ctx(C, H, L, Tb):
    cfg = ML.MmtConfig()
    cfg.num_modalities, cfg.n_embd, cfg.n_head, cfg.n_layer, cfg.block_size = M3, C, H, L, Tb
    for i, v in enumerate(V3):
        cfg.vocab_sizes[i] = v
        cfg.cross_attention[i] = int(CROSS3[i])
    cfg.precision = 0
    ctx = ML.lib().mmt_create(ctypes.byref(cfg))
    assert ctx, ML.lib().mmt_create_error()
    return ctypes.c_void_p(ctx)


def _expected_bytes(C, H, paths, m):
    """include/mmt.h: the compact scratch of one step over paths * m rows (every buffer rounded up to 256 bytes),
    residual rows in two layer slots, and per modality the fp32 [paths, C] rows the post block reads."""
    r8 = lambda x: -(-max(x, 1) // 8) * 8  # noqa: E731
    R = paths * m
    hh = C // H // 2
    ldh1, ldp = r8(3 * H * hh), r8(C // 2)
    total = 0
    for v in V3:
        for n in (R * C * 4, R * C * 2, R * 4, R * 4, R * ldh1 * 2, R * 3 * C * 2, R * C * 2, R * ldp * 2,
                  R * 4 * C * 2, R * C * 2, R * C * 2, R * C * 2, R * C * 2, R * ldp * 2, R * C * 2, R * r8(v // 2) * 2):
            total += _rup(n)
        total += (M3 - 1) * _rup(R * 2 * C * 2)
    total += 2 * M3 * 3 * _rup(R * C * 4)
    total += M3 * _rup(paths * C * 4)
    return total


@pytest.mark.parametrize("C,H,Tb", [(32, 2, 16), (64, 2, 40), (256, 8, 48)])
def test_rolling_bytes_arithmetic_and_no_growth_with_layers(C, H, Tb):
    Lb = ML.lib()
    one, two = _ctx(C, H, 1, Tb), _ctx(C, H, 2, Tb)
    try:
        for B, S, m in ((1, 1, 1), (2, 5, 7), (3, 17, Tb - 1), (1, 4096, 8)):
            want = _expected_bytes(C, H, B * S, m)
            assert Lb.mmt_rolling_bytes(one, B, S, m) == want, (B, S, m)
            assert Lb.mmt_rolling_bytes(two, B, S, m) == want, (B, S, m)  # the tails are per layer in flight
        for B, S, m in ((0, 1, 1), (1, 0, 1), (1, -3, 1), (1, 1, 0), (1, 1, Tb), (1 << 15, 1 << 15, 1)):
            assert Lb.mmt_rolling_bytes(one, B, S, m) == -1, (B, S, m)
        assert Lb.mmt_rolling_bytes(None, 1, 1, 1) == -1
        # monotone in the tail length: a buffer for max_tail serves every shorter tail
        sizes = [Lb.mmt_rolling_bytes(one, 2, 5, m) for m in range(1, Tb)]
        assert sizes == sorted(sizes)
    finally:
        Lb.mmt_destroy(one)
        Lb.mmt_destroy(two)


def test_step_refuses_on_the_host():
    """No forward (MMT_ERR_STATE) and null pointers (MMT_ERR_INVALID) return before any launch, so they need no
    device; the refusals that follow a forward are in tests/test_gpu_rolling_engine.py."""
    Lb = ML.lib()
    ctx = _ctx(32, 2, 1, 16)
    try:
        buf = ctypes.create_string_buffer(64)
        p = ctypes.cast(buf, ctypes.c_void_p)
        arr = (ctypes.c_void_p * 3)(*[p.value] * 3)
        holes = (ctypes.c_void_p * 3)(p.value, 0, p.value)
        step = lambda *a: Lb.mmt_rolling_step(ctx, None, *a)  # noqa: E731
        assert step(2, 3, 5, 4, arr, 9, p, arr, p, p) == -4  # no forward
        assert Lb.mmt_workspace_bytes(ctx, 2) > 0
        assert step(2, 3, 5, 4, arr, 9, p, arr, p, p) == -4  # planned, still no forward
        assert b"mmt_forward" in Lb.mmt_last_error(ctx)
        for args in ((2, 3, 5, 4, None, 9, p, arr, p, p), (2, 3, 5, 4, arr, 9, None, arr, p, p),
                     (2, 3, 5, 4, arr, 9, p, None, p, p), (2, 3, 5, 4, arr, 9, p, arr, None, p),
                     (2, 3, 5, 4, arr, 9, p, arr, p, None), (2, 3, 5, 4, holes, 9, p, arr, p, p),
                     (2, 3, 5, 4, arr, 9, p, holes, p, p)):
            assert step(*args) == -1, args
        assert Lb.mmt_rolling_step(None, None, 2, 3, 5, 4, arr, 9, p, arr, p, p) == -1
    finally:
        Lb.mmt_destroy(ctx)
