"""Host side of generate(num_samples=S), no GPU: argument validation, the row order, the arithmetic of
mmt_fanout_bytes and the refusals of mmt_decode_fanout_step that need no device (mmt_create needs none)."""
import ctypes

import pytest
import torch

import config_utils
import mmt_lib as ML
import model as mmt_model

M3, V3, CROSS3 = 3, [37, 5, 11], [True, False, False]


def _rup(x, a=256):
    return -(-x // a) * a


def _ctx(C, H, L, T, precision=0):
    cfg = ML.MmtConfig()
    cfg.num_modalities, cfg.n_embd, cfg.n_head, cfg.n_layer, cfg.block_size = M3, C, H, L, T
    for i, v in enumerate(V3):
        cfg.vocab_sizes[i] = v
        cfg.cross_attention[i] = int(CROSS3[i])
    cfg.precision = precision
    ctx = ML.lib().mmt_create(ctypes.byref(cfg))
    assert ctx, ML.lib().mmt_create_error()
    return ctypes.c_void_p(ctx)


def _expected_bytes(C, H, L, R, N):
    """include/mmt.h: the compact scratch of one decode step over R rows (every buffer rounded up to 256 bytes),
    then per (layer, modality) a [R, N, 3C] bf16 self-attention tail and, for the cross modality, one [R, N, 2C]
    tail per KV stream."""
    r8 = lambda x: -(-max(x, 1) // 8) * 8  # noqa: E731
    hh = C // H // 2
    ldh1, ldp = r8(3 * H * hh), r8(C // 2)
    total = 0
    for v in V3:
        for n in (R * C * 4, R * C * 2, R * 4, R * 4, R * ldh1 * 2, R * 3 * C * 2, R * C * 2, R * ldp * 2,
                  R * 4 * C * 2, R * C * 2, R * C * 2, R * C * 2, R * C * 2, R * ldp * 2, R * C * 2, R * r8(v // 2) * 2):
            total += _rup(n)
        total += (M3 - 1) * _rup(R * 2 * C * 2)
    total += L * M3 * 3 * _rup(R * C * 4)
    for _ in range(L):
        for cross in CROSS3:
            total += _rup(R * N * 3 * C * 2)
            if cross:
                total += (M3 - 1) * _rup(R * N * 2 * C * 2)
    return total


@pytest.mark.parametrize("C,H,L,T", [(32, 2, 1, 16), (64, 2, 2, 40), (256, 8, 1, 48)])
def test_fanout_bytes_arithmetic(C, H, L, T):
    Lb = ML.lib()
    ctx = _ctx(C, H, L, T)
    try:
        for B, S, N in ((1, 1, 1), (2, 5, 7), (3, 17, T - 1), (1, 4096, 8)):
            assert Lb.mmt_fanout_bytes(ctx, B, S, N) == _expected_bytes(C, H, L, B * S, N), (B, S, N)
        for B, S, N in ((0, 1, 1), (1, 0, 1), (1, -3, 1), (1, 1, 0), (1, 1, T), (1 << 15, 1 << 15, 1)):
            assert Lb.mmt_fanout_bytes(ctx, B, S, N) == -1, (B, S, N)
        assert Lb.mmt_fanout_bytes(None, 1, 1, 1) == -1
        # samples cost the tails and the compact rows, never the workspace: S times the rows of one sample
        one, many = Lb.mmt_fanout_bytes(ctx, 1, 256, 8), Lb.mmt_fanout_bytes(ctx, 256, 1, 8)
        assert one == many
    finally:
        Lb.mmt_destroy(ctx)


def test_step_refuses_on_the_host():
    """No prefill (MMT_ERR_STATE) and null pointers (MMT_ERR_INVALID) return before any launch, so they need no
    device; the refusals that follow a prefill are in tests/test_gpu_decode_fanout.py."""
    Lb = ML.lib()
    ctx = _ctx(32, 2, 1, 16)
    try:
        buf = ctypes.create_string_buffer(64)
        p = ctypes.cast(buf, ctypes.c_void_p)
        arr = (ctypes.c_void_p * 3)(*[p.value] * 3)
        step = lambda *a: Lb.mmt_decode_fanout_step(ctx, None, *a)  # noqa: E731
        assert step(2, 3, 5, 4, 5, arr, p, arr, p, p) == -4  # no prefill
        assert Lb.mmt_workspace_bytes(ctx, 2) > 0
        assert step(2, 3, 5, 4, 5, arr, p, arr, p, p) == -4  # planned, still no prefill
        assert b"prefill" in Lb.mmt_last_error(ctx)
        for args in ((2, 3, 5, 4, 5, None, p, arr, p, p), (2, 3, 5, 4, 5, arr, None, arr, p, p),
                     (2, 3, 5, 4, 5, arr, p, None, p, p), (2, 3, 5, 4, 5, arr, p, arr, None, p),
                     (2, 3, 5, 4, 5, arr, p, arr, p, None)):
            assert step(*args) == -1, args
    finally:
        Lb.mmt_destroy(ctx)


def test_check_num_samples():
    for ok in (1, 2, 4096):
        assert mmt_model.check_num_samples(ok) == ok
    for bad in (0, -1, 1.0, "2", True, False, None):
        with pytest.raises(ValueError):
            mmt_model.check_num_samples(bad)


def test_row_order_is_prompt_major():
    """Row b*S + s is sample s of prompt b: what repeat_interleave gives, which is also the draw key's row."""
    B, S, n0 = 3, 4, 5
    prompts = [torch.arange(B * n0).view(B, n0) + 100 * i for i in range(2)]
    rows = mmt_model.tile_prompts(prompts, S)
    for i, r in enumerate(rows):
        assert tuple(r.shape) == (B * S, n0)
        for b in range(B):
            for s in range(S):
                assert torch.equal(r[b * S + s], prompts[i][b])
    assert all(torch.equal(r, p) for r, p in zip(mmt_model.tile_prompts(prompts, 1), prompts))


def test_generate_validates_num_samples_before_touching_a_device():
    config_utils._config_cache = {"n_embd": 32, "n_head": 4, "n_layer": 1, "block_size": 8, "dropout": 0.0,
                                  "device": "cpu", "batch_size": 2, "eval_iters": 1}
    m = mmt_model.MultimodalTransformer(2, [11, 5], [[None] * 8 + [c] + [None] * 3 for c in (True, False)])
    m.eval()
    assert m.last_generate_path is None
    prompts = [torch.zeros(2, 3, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long)]
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="num_samples"):
            m.generate(prompts, max_new_tokens=2, num_samples=bad)
    with pytest.raises(ValueError, match="sample_fn"):
        m.generate(prompts, max_new_tokens=2, num_samples=3, sample_fn=lambda p: p.argmax(-1, keepdim=True))
    with pytest.raises(RuntimeError, match="ROCm GPU"):  # a CPU-resident model has no path at all, as before
        m.generate(prompts, max_new_tokens=2, num_samples=3)
    assert m.last_generate_path == "tiled"
