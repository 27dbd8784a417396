"""hs-32 self-attention with Q / K / V made on chip (AttnProblem::oc_*, mmt_set_attn_qkv_onchip; include/mmt.h).

Kernel level: mmt_op_attention_fwd_h1 / _bwd_h1 take the stage-1 rows h1 and W2 in place of q / k / v. The
reference is the materialised path on the same inputs: mmt_op_qkv2_fwd, then mmt_op_attention_fwd (the forward:
O and LSE bitwise) or mmt_op_attention_bwd on the one-pass kernel followed by mmt_op_qkv2_bwd (the backward: dh1
and dW2 within GRAD_BOUND, the bound tests/test_gpu_determinism.py states for gradients that differ only in the
order of float atomics). Pad columns of h1 and the rows past the batch hold NaN: nothing may read them.

Engine level: the knob at 1, 2 and 3 against 0 on f_hs32 and f_c1 (forward bitwise, gradient within GRAD_BOUND),
deterministic mode, decode after an eval prefill and after a training forward, and shapes the path must not take.
"""
import ctypes

import pytest
import torch

import mmt_lib as ML
from golden_io import model_fixture, scale_fixture
from test_gpu_determinism import GRAD_BOUND, _build, _fwd_bwd, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 32  # poisoned rows behind the batch (a ragged last tile's rows past T)


def _s():
    return ML.stream_ptr()


def _bf(t):
    return t.to(torch.bfloat16).contiguous()


def _inputs(B, T, H, pad):
    """h1 (NaN in the pad columns and in GUARD rows behind the batch), W2, dO (NaN guard rows)."""
    torch.manual_seed(1000 * B + 10 * T + H + pad)
    R, nblk = B * T, 3 * H
    ld_h1 = nblk * 16 + pad
    h1 = torch.full((R + GUARD, ld_h1), NAN, device=DEV)
    h1[:R, : nblk * 16] = torch.tanh(torch.randn(R, nblk * 16, device=DEV))
    w2 = torch.randn(nblk, 32, 16, device=DEV) * 0.4
    do = torch.full((R + GUARD, H * 32), NAN, device=DEV)
    do[:R] = torch.randn(R, H * 32, device=DEV)
    return _bf(h1), ld_h1, w2, _bf(do)


DROP_P = 0.1
DROP_KEY = 0x0C5EED01


def _dropout(B, T, H):
    """(drop_key, drop_thr, drop_scale, keep-bit buffer) of p = DROP_P, the bits from mmt_op_attention_mask."""
    import attn_drop_ref as DR
    L = ML.lib()
    thr, c = DR.thr_of(DROP_P), DR.scale_of(DROP_P)
    dmask = torch.zeros(L.mmt_op_attention_mask_dwords(B, H, T), dtype=torch.int32, device=DEV)
    mp = (ctypes.c_void_p * 8)(dmask.data_ptr())
    assert L.mmt_op_attention_mask(_s(), 1, B, T, H, (ctypes.c_int32 * 1)(1), (ctypes.c_uint32 * 1)(DROP_KEY),
                                   (ctypes.c_uint32 * 1)(thr), mp) == 0
    torch.cuda.synchronize()
    assert dmask.any()
    return DROP_KEY, thr, c, dmask


def _materialised_forward(B, T, H, h1, ld_h1, w2, drop=None):
    """mmt_op_qkv2_fwd + mmt_op_attention_fwd on clean copies of the rows: qkv, O, LSE."""
    L = ML.lib()
    R, C = B * T, H * 32
    clean = torch.nan_to_num(h1[:R].float(), nan=0.0).to(torch.bfloat16).contiguous()
    qkv = torch.zeros(R, 3 * C, dtype=torch.bfloat16, device=DEV)
    assert L.mmt_op_qkv2_fwd(_s(), R, 3 * H, 32, ML.ptr(clean), ld_h1, ML.ptr(w2), ML.ptr(qkv), 3 * C) == 0
    o = torch.zeros(R, C, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B * H * T, device=DEV)
    kp = (ctypes.c_void_p * 1)(qkv.data_ptr())
    vp = (ctypes.c_void_p * 1)(qkv[:, 2 * C:].data_ptr())
    args = (_s(), B, T, H, 32, 1, ML.ptr(qkv[:, C:]), 3 * C, kp, vp, 3 * C, 32, ML.ptr(o), C, None, ML.ptr_array([lse]))
    if drop is None:
        assert L.mmt_op_attention_fwd(*args) == 0
    else:
        assert L.mmt_op_attention_fwd_drop(*args, drop[0], drop[1], drop[2], (ctypes.c_void_p * 1)(drop[3].data_ptr())) == 0
    torch.cuda.synchronize()
    return clean, qkv, o, lse


# (2, 256, 8): all eight tiles, every wave with two; (3, 37, 2): ragged second tile; (1, 33, 2): one row past a
# tile edge; (1, 2, 2): a single partial tile; (2, 96, 1): waves with zero or one tile, ld_h1 = 48.
# pad 8: ld_h1 has 8 pad columns (NaN) behind the 3 H 16 used ones
SHAPES = [(2, 256, 8), (3, 37, 2), (1, 33, 2), (1, 2, 2), (2, 96, 1)]


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("B,T,H", SHAPES)
def test_forward_from_h1_same_bits_as_materialised(B, T, H, pad, drop=None):
    """O and LSE against mmt_op_qkv2_fwd + mmt_op_attention_fwd, bitwise. (The hs-32 stage-2 kernel behind
    mmt_op_qkv2_fwd feeds its MFMA in the K-slot order of the stage-1 GEMM's epilogue, as the on-chip kernels do: in
    the natural order its rows differed from the epilogue's by one bf16 ulp in 2 of 393216 entries at (2, 256, 8),
    and O with them, max |dO| 2.5e-5.)"""
    L = ML.lib()
    R, C = B * T, H * 32
    h1, ld_h1, w2, _ = _inputs(B, T, H, pad)
    _, _, o_ref, lse_ref = _materialised_forward(B, T, H, h1, ld_h1, w2, drop)
    o = torch.zeros(R + GUARD, C, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B * H * T, device=DEV)
    args = (_s(), B, T, H, ML.ptr(h1), ld_h1, ML.ptr(w2), ML.ptr(o), C, ML.ptr(lse))
    if drop is None:
        assert L.mmt_op_attention_fwd_h1(*args) == 0
    else:
        assert L.mmt_op_attention_fwd_h1_drop(*args, drop[0], drop[1], drop[2], ML.ptr(drop[3])) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert o_ref.float().abs().max() > 0
    assert torch.equal(o[:R], o_ref), (o[:R].float() - o_ref.float()).abs().max().item()
    assert torch.equal(lse, lse_ref), (lse - lse_ref).abs().max().item()
    assert not o[R:].float().any()  # nothing written behind the batch


@pytest.mark.parametrize("B,T,H", SHAPES)
def test_forward_from_h1_same_bits_as_gemm_epilogue_rows(B, T, H):
    """The rows the engine materialises come from the stage-1 GEMM's fused epilogue (mmt_op_gemm_qkv): h1 and Q/K/V
    from one launch, the attention forward over those rows, and the on-chip forward over that h1: O and LSE bitwise;
    and mmt_op_qkv2_fwd on that h1 gives the epilogue's Q/K/V rows bit for bit."""
    L = ML.lib()
    torch.manual_seed(7 * B + T + H)
    R, C, N, K = B * T, H * 32, 3 * H * 16, 64
    X = _bf(torch.randn(R, K, device=DEV))
    W1 = _bf(torch.randn(N, K, device=DEV) / K ** 0.5)
    b1 = torch.randn(N, device=DEV) * 0.3
    w2 = torch.randn(3 * H, 32, 16, device=DEV) * 0.4
    h1 = torch.full((R + GUARD, N), NAN, dtype=torch.bfloat16, device=DEV)
    qkv = torch.zeros(R, 3 * C, dtype=torch.bfloat16, device=DEV)
    assert L.mmt_op_gemm_qkv(_s(), R, N, K, ML.ptr(X), K, ML.ptr(W1), K, ML.ptr(b1), ML.ptr(h1), N, ML.ptr(w2), 16,
                             ML.ptr(qkv), 3 * C) == 0
    o_ref = torch.zeros(R, C, dtype=torch.bfloat16, device=DEV)
    lse_ref = torch.zeros(B * H * T, device=DEV)
    kp = (ctypes.c_void_p * 1)(qkv.data_ptr())
    vp = (ctypes.c_void_p * 1)(qkv[:, 2 * C:].data_ptr())
    assert L.mmt_op_attention_fwd(_s(), B, T, H, 32, 1, ML.ptr(qkv[:, C:]), 3 * C, kp, vp, 3 * C, 32, ML.ptr(o_ref), C,
                                  None, ML.ptr_array([lse_ref])) == 0
    o = torch.zeros(R, C, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B * H * T, device=DEV)
    assert L.mmt_op_attention_fwd_h1(_s(), B, T, H, ML.ptr(h1), N, ML.ptr(w2), ML.ptr(o), C, ML.ptr(lse)) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(h1[:R].float()).all() and o_ref.float().abs().max() > 0
    assert torch.equal(o, o_ref), (o.float() - o_ref.float()).abs().max().item()
    assert torch.equal(lse, lse_ref), (lse - lse_ref).abs().max().item()
    rows = torch.zeros_like(qkv)
    assert L.mmt_op_qkv2_fwd(_s(), R, 3 * H, 32, ML.ptr(h1), N, ML.ptr(w2), ML.ptr(rows), 3 * C) == 0
    torch.cuda.synchronize()
    assert torch.equal(rows, qkv), int((rows != qkv).sum())


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("B,T,H", SHAPES)
def test_backward_from_h1_matches_materialised(B, T, H, pad, drop=None):
    L = ML.lib()
    R, C, nblk = B * T, H * 32, 3 * H
    h1, ld_h1, w2, do = _inputs(B, T, H, pad)
    clean, qkv, o, lse = _materialised_forward(B, T, H, h1, ld_h1, w2, drop)
    # reference: the one-pass backward (mmt_attn_set_ring bit 6) writes bf16 dQ / dK / dV, then the stage-2 backward
    old = L.mmt_attn_set_ring(15 | 64)
    try:
        dqkv = torch.zeros(R, 3 * C, dtype=torch.bfloat16, device=DEV)
        dvec = torch.zeros(B * H * T, device=DEV)
        kp = (ctypes.c_void_p * 1)(qkv.data_ptr())
        vp = (ctypes.c_void_p * 1)(qkv[:, 2 * C:].data_ptr())
        dkp = (ctypes.c_void_p * 1)(dqkv.data_ptr())
        dvp = (ctypes.c_void_p * 1)(dqkv[:, 2 * C:].data_ptr())
        do_clean = do[:R].contiguous()
        args = (_s(), B, T, H, 32, 1, ML.ptr(qkv[:, C:]), 3 * C, kp, vp, 3 * C, 32, ML.ptr(o), C, None,
                ML.ptr_array([lse]), ML.ptr(do_clean), C, ML.ptr_array([dvec]), ML.ptr(dqkv[:, C:]), 3 * C, dkp, dvp,
                3 * C, 32)
        if drop is None:
            assert L.mmt_op_attention_bwd(*args) == 0
        else:
            assert L.mmt_op_attention_bwd_drop(*args, None, 0, drop[0], drop[1], drop[2],
                                               (ctypes.c_void_p * 1)(drop[3].data_ptr())) == 0
        dh1_ref = torch.zeros(R, ld_h1, dtype=torch.bfloat16, device=DEV)
        dw2_ref = torch.zeros_like(w2)
        assert L.mmt_op_qkv2_bwd(_s(), R, nblk, 32, ML.ptr(clean), ld_h1, ML.ptr(w2), ML.ptr(dqkv), 3 * C,
                                 ML.ptr(dh1_ref), ML.ptr(dw2_ref)) == 0
        # under test: O and LSE with poisoned guard rows behind them
        o_g = torch.full((R + GUARD, C), NAN, dtype=torch.bfloat16, device=DEV)
        o_g[:R] = o
        lse_g = torch.full((B * H * T + GUARD,), NAN, device=DEV)
        lse_g[: B * H * T] = lse
        dh1 = torch.zeros(R + GUARD, ld_h1, dtype=torch.bfloat16, device=DEV)
        dw2 = torch.zeros_like(w2)
        db1 = torch.zeros(nblk * 16, device=DEV)
        args = (_s(), B, T, H, ML.ptr(h1), ld_h1, ML.ptr(w2), ML.ptr(o_g), C, ML.ptr(lse_g), ML.ptr(do), C, ML.ptr(dh1),
                ML.ptr(dw2), ML.ptr(db1))
        if drop is None:
            assert L.mmt_op_attention_bwd_h1(*args) == 0
        else:
            assert L.mmt_op_attention_bwd_h1_drop(*args, drop[0], drop[1], drop[2], ML.ptr(drop[3])) == 0
        torch.cuda.synchronize()
    finally:
        L.mmt_attn_set_ring(old)
    for t in (dh1, dw2, db1):
        assert torch.isfinite(t.float()).all()
    assert dh1_ref.float().abs().max() > 0 and dw2_ref.abs().max() > 0
    e_h, e_w = _rel(dh1[:R].float(), dh1_ref.float()), _rel(dw2, dw2_ref)
    print(f"B {B} T {T} H {H} pad {pad}: dh1 rel-L2 {e_h:.3e}, dW2 rel-L2 {e_w:.3e}")
    assert e_h <= GRAD_BOUND, e_h
    assert e_w <= GRAD_BOUND, e_w
    assert not dh1[R:].float().any() and not dh1[:, nblk * 16:].float().any()  # guard rows, pad columns untouched
    # db1 = the column sums of dh1 before its bf16 rounding: every entry of dh1 is within half a bf16 ulp (2^-8
    # relative) of its fp32 value, so each sum is within 2^-8 of the column's absolute sum (+ fp32 summation slack)
    cols = dh1[:R, : nblk * 16].float()
    slack = cols.abs().sum(0) * (2.0 ** -8 + 1e-5) + 1e-6
    assert ((db1 - cols.sum(0)).abs() <= slack).all(), ((db1 - cols.sum(0)).abs() / slack).max().item()


# the smallest shape and T = 256, under dropout of the probabilities (p = 0.1): both paths read the same keep bits
DROP_SHAPES = [(1, 2, 2), (2, 256, 8)]


@pytest.mark.parametrize("B,T,H", DROP_SHAPES)
def test_forward_from_h1_dropout_same_bits_as_materialised(B, T, H):
    """mmt_op_attention_fwd_h1_drop against mmt_op_attention_fwd_drop on the materialised Q/K/V: O and LSE bitwise,
    and the mask acts (O differs from the forward without dropout)."""
    drop = _dropout(B, T, H)
    test_forward_from_h1_same_bits_as_materialised(B, T, H, 8, drop)
    h1, ld_h1, w2, _ = _inputs(B, T, H, 8)
    _, _, o_drop, lse_drop = _materialised_forward(B, T, H, h1, ld_h1, w2, drop)
    _, _, o_plain, lse_plain = _materialised_forward(B, T, H, h1, ld_h1, w2)
    assert not torch.equal(o_drop, o_plain) and torch.equal(lse_drop, lse_plain)


@pytest.mark.parametrize("B,T,H", DROP_SHAPES)
def test_backward_from_h1_dropout_matches_materialised(B, T, H):
    """mmt_op_attention_bwd_h1_drop against the materialised one-pass backward with the same keep bits, at
    test_backward_from_h1_matches_materialised's bounds."""
    test_backward_from_h1_matches_materialised(B, T, H, 8, _dropout(B, T, H))


def test_unsupported_shapes_are_refused_not_run():
    L = ML.lib()
    B, T, H = 1, 300, 2  # T > 256
    h1, ld_h1, w2, do = _inputs(B, T, H, 0)
    o = torch.zeros(B * T, H * 32, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B * H * T, device=DEV)
    assert L.mmt_op_attention_fwd_h1(_s(), B, T, H, ML.ptr(h1), ld_h1, ML.ptr(w2), ML.ptr(o), H * 32, ML.ptr(lse)) == -2
    dh1 = torch.zeros(B * T, ld_h1, dtype=torch.bfloat16, device=DEV)
    dw2, db1 = torch.zeros_like(w2), torch.zeros(3 * H * 16, device=DEV)
    assert L.mmt_op_attention_bwd_h1(_s(), B, T, H, ML.ptr(h1), ld_h1, ML.ptr(w2), ML.ptr(o), H * 32, ML.ptr(lse),
                                     ML.ptr(do), H * 32, ML.ptr(dh1), ML.ptr(dw2), ML.ptr(db1)) == -2
    # a row stride that is no multiple of 8
    assert L.mmt_op_attention_fwd_h1(_s(), 1, 32, H, ML.ptr(h1), ld_h1 + 4, ML.ptr(w2), ML.ptr(o), H * 32, ML.ptr(lse)) == -2
    torch.cuda.synchronize()
    assert not o.float().any() and not dh1.float().any() and not dw2.any()


# ------------------------------------------------------------------------------------------------ engine level
def _fixture(name):
    return scale_fixture(name) if name == "f_c1" else model_fixture(name)


_STEPS = {}


def _step(name, dropout, knob, det=False):
    """(logits, losses, gradient) of one fixture step with the knob at `knob` (a fresh model each; knob 0 is
    computed once per (fixture, dropout, mode) and shared)."""
    key = (name, dropout, knob, det)
    if key in _STEPS:
        return _STEPS[key]
    L = ML.lib()
    z, meta, cfg, sd, idx, tgt = _fixture(name)
    old = L.mmt_set_attn_qkv_onchip(knob)
    try:
        m = _build(meta, sd, dropout)
        m.set_deterministic(det)
        out = _fwd_bwd(m, [t.cuda() for t in idx], [t.cuda() for t in tgt])
    finally:
        L.mmt_set_attn_qkv_onchip(old)
    if knob == 0:
        _STEPS[key] = out
    return out


@pytest.mark.parametrize("knob", [3, 1, 2])
@pytest.mark.parametrize("dropout", [0.1, 0.0])
@pytest.mark.parametrize("name", ["f_hs32", "f_c1"])
def test_engine_knob_matches_materialised(name, dropout, knob):
    """Forward bitwise (the same Q/K/V bits reach the same attention arithmetic), gradient within GRAD_BOUND (the
    stage-2 sums are the only float atomics involved, and their order is all that moves)."""
    assert _fixture(name)[1]["n_embd"] // _fixture(name)[1]["n_head"] == 32
    lg0, ls0, g0 = _step(name, dropout, 0)
    lg1, ls1, g1 = _step(name, dropout, knob)
    assert torch.equal(ls0, ls1), (ls0, ls1)
    for a, b in zip(lg0, lg1):
        assert torch.equal(a, b)
    err = _rel(g1, g0)
    print(f"{name} dropout {dropout} knob {knob}: grad rel-L2 vs knob 0 {err:.3e}")
    assert torch.isfinite(g1).all() and g0.abs().max() > 0
    assert err <= GRAD_BOUND, err


def test_engine_deterministic_mode_same_bits_twice():
    L = ML.lib()
    z, meta, cfg, sd, idx, tgt = model_fixture("f_hs32")
    old = L.mmt_set_attn_qkv_onchip(3)
    try:
        m = _build(meta, sd, 0.1)
        m.set_deterministic(True)
        idx_d, tgt_d = [t.cuda() for t in idx], [t.cuda() for t in tgt]
        a = _fwd_bwd(m, idx_d, tgt_d)
        b = _fwd_bwd(m, idx_d, tgt_d)
    finally:
        L.mmt_set_attn_qkv_onchip(old)
    assert torch.equal(a[1], b[1])
    assert torch.equal(a[2], b[2]), _rel(a[2], b[2])
    # and the deterministic gradient is the materialised path's: no sum was added or reordered
    ref = _step("f_hs32", 0.1, 0, det=True)
    assert torch.equal(a[1], ref[1])
    assert torch.equal(a[2], ref[2]), _rel(a[2], ref[2])


def test_decode_after_eval_prefill_still_matches_full_forward():
    """An eval prefill is a training == 0 forward: it writes Q/K/V (the decode cache) whatever the knob says."""
    L = ML.lib()
    z, meta, cfg, sd, idx, tgt = model_fixture("f_hs32")
    old = L.mmt_set_attn_qkv_onchip(3)
    try:
        m = _build(meta, sd, 0.1)
        m.eval()
        T = meta["block_size"]
        P = max(1, T // 2 - 1)
        seq = [t.cuda() for t in idx]
        with torch.no_grad():
            m([s[:, :P] for s in seq])
            dec = [m._decode_step([s[:, t] for s in seq], t) for t in range(P, T)]
            full, _ = m(seq)
    finally:
        L.mmt_set_attn_qkv_onchip(old)
    for i in range(len(meta["V"])):
        got = torch.stack([d[i] for d in dec], dim=1)
        assert _rel(got.float(), full[i][:, P:T].float()) < 1e-2  # the bound of test_kv_cache_decode_matches_full_forward


def test_decode_after_training_forward_is_refused():
    L = ML.lib()
    z, meta, cfg, sd, idx, tgt = model_fixture("f_hs32")
    old = L.mmt_set_attn_qkv_onchip(3)
    try:
        m = _build(meta, sd, 0.1)  # train mode with dropout: training = 1
        seq = [t.cuda() for t in idx]
        with torch.no_grad():
            m(seq, [t.cuda() for t in tgt])
            with pytest.raises(ML.MmtError, match=r"status -1\).*on\s+chip"):
                m._decode_step([s[:, 1] for s in seq], 1)
            m.eval()
            m([s[:, :4] for s in seq])  # an eval prefill re-arms the cache
            m._decode_step([s[:, 4] for s in seq], 4)
    finally:
        L.mmt_set_attn_qkv_onchip(old)


def _hs64_fixture():
    import mmt_oracle as O
    H, L_, T, B = 2, 2, 40, 3
    C, V, cross = H * 64, [37, 5, 11], [True, False, False]
    cfg = O.OracleConfig(C, H, L_, T, V, cross)
    g = torch.Generator().manual_seed(64)
    sd = O.init_params(cfg, g)
    tril = [f"blocks.{l}.{kind}.{i}.heads.{h}.tril" for l in range(L_) for i in range(len(V))
            for kind in ("sa_layers", "cross_attention_layers") for h in range(H) if kind == "sa_layers" or cross[i]]
    meta = {"n_embd": C, "n_head": H, "n_layer": L_, "block_size": T, "B": B, "V": V, "cross": cross,
            "state_dict_keys": list(sd.keys()) + tril}
    idx = [torch.randint(0, v, (B, T), generator=g) for v in V]
    tgt = [torch.randint(0, v, (B, T), generator=g) for v in V]
    return meta, sd, idx, tgt


@pytest.mark.parametrize("name", ["f_small", "hs64"])
def test_other_head_sizes_do_not_take_the_path(name):
    """hs 16 (f_small) and hs 64: knob 3 changes nothing. Deterministic mode, so the gradients compare bitwise."""
    L = ML.lib()
    if name == "hs64":
        meta, sd, idx, tgt = _hs64_fixture()
    else:
        z, meta, cfg, sd, idx, tgt = model_fixture(name)
    assert meta["n_embd"] // meta["n_head"] != 32
    out = {}
    for knob in (0, 3):
        old = L.mmt_set_attn_qkv_onchip(knob)
        try:
            m = _build(meta, sd, 0.1)
            m.set_deterministic(True)
            out[knob] = _fwd_bwd(m, [t.cuda() for t in idx], [t.cuda() for t in tgt])
            with torch.no_grad():  # and the training forward left a K/V cache behind: decode is refused only for dropout
                with pytest.raises(ML.MmtError, match="dropout"):
                    m._decode_step([s[:, 1].cuda() for s in idx], 1)
        finally:
            L.mmt_set_attn_qkv_onchip(old)
    assert torch.equal(out[0][1], out[3][1])
    for a, b in zip(out[0][0], out[3][0]):
        assert torch.equal(a, b)
    assert torch.equal(out[0][2], out[3][2]), _rel(out[3][2], out[0][2])
