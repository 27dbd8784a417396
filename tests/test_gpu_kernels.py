"""Kernel-level parity: each HIP kernel (through the C-ABI mmt_op_* entry points) against a plain
PyTorch fp32 reference of the same op on the same bf16-rounded inputs.

Tolerances: fp32 outputs of bf16 MFMA products accumulate exactly-representable products in fp32,
so they match an fp32 reference to ~1e-5 relative; bf16 outputs carry one bf16 rounding
(rel 2^-8 = 3.9e-3) on top.
"""
import ctypes

import pytest
import torch

import attn_plan as AP
import mmt_lib as ML

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _s():
    return ML.stream_ptr()


def _sync():
    torch.cuda.synchronize()


def rel(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def bf(t):
    return t.to(torch.bfloat16).contiguous()


def pad_cols(t, ld):
    out = torch.zeros(t.shape[0], ld, dtype=t.dtype, device=t.device)
    out[:, : t.shape[1]] = t
    return out


def r8(x):
    return max(8, (x + 7) // 8 * 8)


# ------------------------------------------------------------------------------------- GEMM
# the last three take the 256x256-tile kernel (M, N >= 256 and K >= 512), one with ragged edges
GEMM_SHAPES = [(256, 128, 64), (200, 136, 72), (33, 17, 45), (128, 450, 256), (5, 900, 450), (16384 // 64, 384, 256),
               (512, 256, 512), (300, 264, 520), (1024, 1024, 1024)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("epi", ["store_bf16", "bias_tanh_bf16", "bias_relu_bf16", "bias_resid_f32", "store_f32"])
def test_gemm_forward_linear(M, N, K, epi):
    torch.manual_seed(M * 7 + N + K)
    lda, ldb = r8(K), r8(K)
    X = torch.randn(M, K, device=DEV)
    W = torch.randn(N, K, device=DEV) * 0.1
    bias = torch.randn(N, device=DEV)
    resid = torch.randn(M, N, device=DEV)
    Xb, Wb = bf(pad_cols(X, lda)), bf(pad_cols(W, ldb))
    ref = Xb.float()[:, :K] @ Wb.float()[:, :K].t()
    ldc = N
    ldo16 = r8(N)
    o32 = torch.zeros(M, ldc, device=DEV)
    o16 = torch.zeros(M, ldo16, dtype=torch.bfloat16, device=DEV)
    use_bias = epi != "store_bf16"
    rc = ML.lib().mmt_op_gemm(_s(), 1, 1, ML.EPI[epi], 1, M, N, K, ML.ptr(Xb), lda, ML.ptr(Wb), ldb,
                              ML.ptr(bias) if use_bias else None, None, 0, ML.ptr(resid), N, ML.ptr(o32), ldc,
                              ML.ptr(o16), ldo16, 1.0)
    assert rc == 0
    _sync()
    if use_bias:
        ref = ref + bias
    if epi == "bias_tanh_bf16":
        assert rel(o16[:, :N], torch.tanh(ref)) < 1e-2
    elif epi == "bias_relu_bf16":
        assert rel(o16[:, :N], torch.relu(ref)) < 1e-2
    elif epi == "store_bf16":
        assert rel(o16[:, :N], ref) < 1e-2
    elif epi == "bias_resid_f32":
        assert rel(o32, ref + resid) < 1e-5
    else:
        assert rel(o32, ref) < 1e-5


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (200, 72, 136), (64, 450, 900), (33, 45, 17), (512, 512, 512),
                                   (300, 264, 600)])
@pytest.mark.parametrize("epi", ["dtanh_bf16", "drelu_bf16", "store_f32", "acc_f32", "store_bf16"])
def test_gemm_backward_data(M, N, K, epi):
    # dX[M, N] = dY[M, K] @ W[K, N]  (W stored [K rows][N cols], N contiguous)
    torch.manual_seed(M + 3 * N + K)
    lda, ldb = r8(K), r8(N)
    dY = torch.randn(M, K, device=DEV)
    W = torch.randn(K, N, device=DEV) * 0.1
    aux = torch.tanh(torch.randn(M, N, device=DEV)) if epi != "drelu_bf16" else torch.randn(M, N, device=DEV)
    dYb, Wb = bf(pad_cols(dY, lda)), bf(pad_cols(W, ldb))
    auxb = bf(pad_cols(aux, r8(N)))
    ref = 0.5 * (dYb.float()[:, :K] @ Wb.float()[:, :N])
    o32 = torch.randn(M, N, device=DEV)
    base = o32.clone()
    o16 = torch.zeros(M, r8(N), dtype=torch.bfloat16, device=DEV)
    rc = ML.lib().mmt_op_gemm(_s(), 1, 0, ML.EPI[epi], 1, M, N, K, ML.ptr(dYb), lda, ML.ptr(Wb), ldb, None,
                              ML.ptr(auxb), r8(N), None, 0, ML.ptr(o32), N, ML.ptr(o16), r8(N), 0.5)
    assert rc == 0
    _sync()
    a = auxb.float()[:, :N]
    if epi == "dtanh_bf16":
        assert rel(o16[:, :N], ref * (1 - a * a)) < 1e-2
    elif epi == "drelu_bf16":
        assert rel(o16[:, :N], ref * (a > 0)) < 1e-2
    elif epi == "store_bf16":
        assert rel(o16[:, :N], ref) < 1e-2
    elif epi == "store_f32":
        assert rel(o32, ref) < 1e-5
    else:
        assert rel(o32, base + ref) < 1e-5


@pytest.mark.parametrize("variant", [0x100 | 0x10000, 0x200 | 0x10000, 0x300 | 0x10000, 0x10000, 5, 2, 4, 0x20000 | 0x10000])
@pytest.mark.parametrize("M,N,K", [(512, 256, 512), (300, 264, 520), (768, 520, 136), (256, 1024, 64),
                                   (520, 776, 1000), (256, 256, 32)])
def test_gemm_pipeline_variants(variant, M, N, K):
    """The 256 x 256 tile's rings (BK 32 x 4, BK 32 x 3, BK 32 x 2, BK 64 x 2: bits 8-11, forced at every K by bit
    16), the ping-pong 256 x 256 kernel (gemm8_kernel, bit 17: K-tiles 1, 2, 3, 8, 9 and 16, ragged M / N / K)
    and the deeper 128 x 128 rings (variants 5 / 2 / 4) on the forward and backward-data epilogues,
    ragged edges included (the rings' vmcnt counts depend on the stages left in flight)."""
    L = ML.lib()
    assert L.mmt_gemm_set_variant(variant) == 0
    try:
        for epi in ["store_bf16", "bias_tanh_bf16", "bias_relu_bf16", "bias_resid_f32", "store_f32"]:
            test_gemm_forward_linear(M, N, K, epi)
        for epi in ["store_bf16", "dtanh_bf16", "drelu_bf16", "store_f32", "acc_f32"]:
            test_gemm_backward_data(M, N, K, epi)
    finally:
        L.mmt_gemm_set_variant(-1)


@pytest.mark.parametrize("M,N,K", [(512, 256, 512), (300, 264, 520), (768, 520, 136), (256, 1024, 64),
                                   (520, 776, 1000), (256, 256, 32), (1000, 600, 512)])
def test_gemm_t2_tile(M, N, K):
    """The 128 x 256 tile at two workgroups per CU (mmt_gemm_set_t2(1): the big launches with K below 1024;
    bit 16 of the variant forces the big path at every K) on every forward and backward-data epilogue,
    ragged M / N / K included."""
    L = ML.lib()
    assert L.mmt_gemm_set_variant(0x10000) == 0
    old = L.mmt_gemm_set_t2(1)
    try:
        for epi in ["store_bf16", "bias_tanh_bf16", "bias_relu_bf16", "bias_resid_f32", "store_f32"]:
            test_gemm_forward_linear(M, N, K, epi)
        for epi in ["store_bf16", "dtanh_bf16", "drelu_bf16", "store_f32", "acc_f32"]:
            test_gemm_backward_data(M, N, K, epi)
    finally:
        L.mmt_gemm_set_t2(old)
        L.mmt_gemm_set_variant(-1)


@pytest.mark.parametrize("M,N,R", [(384, 256, 4096), (1024, 256, 2048), (900, 450, 1000), (6, 32, 300), (32, 16, 77)])
@pytest.mark.parametrize("splits", [1, 4, 0])
def test_gemm_weight_grad(M, N, R, splits):
    # dW[M, N] += alpha * dY[R, M]^T @ X[R, N]
    torch.manual_seed(M + N + R + splits)
    lda, ldb = r8(M), r8(N)
    dY = torch.randn(R, M, device=DEV)
    X = torch.randn(R, N, device=DEV)
    dYb, Xb = bf(pad_cols(dY, lda)), bf(pad_cols(X, ldb))
    ref = 0.25 * (dYb.float()[:, :M].t() @ Xb.float()[:, :N])
    out = torch.ones(M, N, device=DEV)
    rc = ML.lib().mmt_op_gemm(_s(), 0, 0, ML.EPI["atomic_f32"], splits, M, N, R, ML.ptr(dYb), lda, ML.ptr(Xb), ldb,
                              None, None, 0, None, 0, ML.ptr(out), N, None, 0, 0.25)
    assert rc == 0
    _sync()
    assert rel(out - 1.0, ref) < 1e-5


@pytest.mark.parametrize("M,N,R", [(1024, 256, 16384), (384, 256, 4096), (900, 450, 1000), (6, 32, 300),
                                   (128, 256, 16384), (450, 256, 3000)])
@pytest.mark.parametrize("slab_mb", [0, 64])
@pytest.mark.parametrize("variant", [-1, 0x30000, 0x300])
def test_gemm_wgrad_slabs(M, N, R, slab_mb, variant):
    # the engine's weight-gradient path: split-K fp32 slabs + reduce (or one K pass without scratch);
    # variant 0x30000: the ping-pong 256 x 256 kernel (MN-contiguous operands, K slices, XCD-major grid);
    # 0x300: the 256 x 256 ring at BK 32 x 2 stages
    L = ML.lib()
    assert L.mmt_gemm_set_variant(variant) == 0
    try:
        _wgrad_slabs(M, N, R, slab_mb)
    finally:
        L.mmt_gemm_set_variant(-1)


def _wgrad_slabs(M, N, R, slab_mb):
    torch.manual_seed(M + 2 * N + R)
    lda, ldb = r8(M), r8(N)
    dY = torch.randn(R, M, device=DEV)
    X = torch.randn(R, N, device=DEV)
    dYb, Xb = bf(pad_cols(dY, lda)), bf(pad_cols(X, ldb))
    ref = 0.25 * (dYb.float()[:, :M].t() @ Xb.float()[:, :N])
    out = torch.ones(M, N, device=DEV)
    slab = torch.empty(slab_mb << 20, dtype=torch.uint8, device=DEV) if slab_mb else None
    rc = ML.lib().mmt_op_gemm_wgrad(_s(), M, N, R, ML.ptr(dYb), lda, ML.ptr(Xb), ldb, ML.ptr(out), N, 0.25,
                                    ML.ptr(slab), slab_mb << 20)
    assert rc == 0
    _sync()
    assert rel(out - 1.0, ref) < 1e-5


def test_gemm_identity_asymmetric():
    # A = I with an asymmetric B catches a transposed C write (guide §3)
    n = 64
    A = torch.eye(n, device=DEV)
    Bm = torch.arange(n * n, device=DEV, dtype=torch.float32).view(n, n) % 17 - 8
    o32 = torch.zeros(n, n, device=DEV)
    Ab, Bb = bf(A), bf(Bm)  # keep both alive for the launch
    rc = ML.lib().mmt_op_gemm(_s(), 1, 1, ML.EPI["store_f32"], 1, n, n, n, ML.ptr(Ab), n, ML.ptr(Bb), n, None,
                              None, 0, None, 0, ML.ptr(o32), n, None, 0, 1.0)
    assert rc == 0
    _sync()
    torch.testing.assert_close(o32, Bm.t().contiguous())


def test_gemm_identity_asymmetric_big_tile():
    # the same transposition check through the 256x256-tile kernel: A = [I | 0] (K = 512)
    n, k = 256, 512
    A = torch.zeros(n, k, device=DEV)
    A[:, :n] = torch.eye(n, device=DEV)
    Bm = torch.arange(n * k, device=DEV, dtype=torch.float32).view(n, k) % 17 - 8
    o32 = torch.zeros(n, n, device=DEV)
    Ab, Bb = bf(A), bf(Bm)
    rc = ML.lib().mmt_op_gemm(_s(), 1, 1, ML.EPI["store_f32"], 1, n, n, k, ML.ptr(Ab), k, ML.ptr(Bb), k, None,
                              None, 0, None, 0, ML.ptr(o32), n, None, 0, 1.0)
    assert rc == 0
    _sync()
    torch.testing.assert_close(o32, Bm[:, :n].t().contiguous())


def test_gemm8_identity_asymmetric():
    # transposition check through the ping-pong kernel (16x16x32 accumulator layout), both W layouts
    n, k = 256, 512
    L = ML.lib()
    assert L.mmt_gemm_set_variant(0x20000 | 0x10000) == 0
    try:
        A = torch.zeros(n, k, device=DEV)
        A[:, :n] = torch.eye(n, device=DEV)
        Bm = torch.arange(n * k, device=DEV, dtype=torch.float32).view(n, k) % 17 - 8
        o32 = torch.zeros(n, n, device=DEV)
        Ab, Bb = bf(A), bf(Bm)
        assert L.mmt_op_gemm(_s(), 1, 1, ML.EPI["store_f32"], 1, n, n, k, ML.ptr(Ab), k, ML.ptr(Bb), k, None,
                             None, 0, None, 0, ML.ptr(o32), n, None, 0, 1.0) == 0
        _sync()
        torch.testing.assert_close(o32, Bm[:, :n].t().contiguous())
        # backward-data form: W stored [K][N]; out = A @ W = W[:n, :]
        Wk = bf(torch.arange(k * n, device=DEV, dtype=torch.float32).view(k, n) % 13 - 6)
        o32.zero_()
        assert L.mmt_op_gemm(_s(), 1, 0, ML.EPI["store_f32"], 1, n, n, k, ML.ptr(Ab), k, ML.ptr(Wk), n, None,
                             None, 0, None, 0, ML.ptr(o32), n, None, 0, 1.0) == 0
        _sync()
        torch.testing.assert_close(o32, Wk.float()[:n, :])
    finally:
        L.mmt_gemm_set_variant(-1)


@pytest.mark.parametrize("which", ["fwd", "dx", "dw"])
def test_gemm_operand_beyond_2gib(which):
    """buffer offsets are 32-bit, so a descriptor anchored at a whole operand read zeros past
    2 GiB. The descriptors now start at the tile's first row (K-contiguous operands) or the K-step's first
    row (MN-contiguous ones): an operand of 2.25 GiB gives the same products as torch on rows past the
    boundary (forward, backward-data) and on the whole weight gradient."""
    torch.manual_seed(11)
    K = 1024
    M = (1 << 20) + 65536  # M x K bf16 = 2.25 GiB
    L = ML.lib()
    if which in ("fwd", "dx"):
        A = torch.empty(M, K, dtype=torch.bfloat16, device=DEV)
        A.uniform_(-1, 1)
        N = 256
        W = bf(torch.randn(N, K, device=DEV) * 0.05) if which == "fwd" else bf(torch.randn(K, N, device=DEV) * 0.05)
        o16 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        rc = L.mmt_op_gemm(_s(), 1, 1 if which == "fwd" else 0, ML.EPI["store_bf16"], 1, M, N, K, ML.ptr(A), K,
                           ML.ptr(W), K if which == "fwd" else N, None, None, 0, None, 0, None, 0, ML.ptr(o16), N, 1.0)
        assert rc == 0
        _sync()
        Wf = W.float().t() if which == "fwd" else W.float()
        # rows either side of the 2 GiB byte offset of A, and the last rows
        edge = (1 << 31) // (2 * K)
        for r0 in (0, edge - 256, edge, M - 512):
            ref = A[r0:r0 + 512].float() @ Wf
            assert rel(o16[r0:r0 + 512], ref) < 1e-2, r0
    else:
        # dW[Mw, N] = dY[R, Mw]^T X[R, N] with dY of 2.25 GiB (K = R rows, MN-contiguous operands)
        R, Mw, N = M, K, 64
        dY = torch.empty(R, Mw, dtype=torch.bfloat16, device=DEV)
        dY.uniform_(-1, 1)
        X = torch.empty(R, N, dtype=torch.bfloat16, device=DEV)
        X.uniform_(-1, 1)
        out = torch.zeros(Mw, N, device=DEV)
        slab = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)
        rc = L.mmt_op_gemm_wgrad(_s(), Mw, N, R, ML.ptr(dY), Mw, ML.ptr(X), N, ML.ptr(out), N, 1.0, ML.ptr(slab),
                                 256 << 20)
        assert rc == 0
        _sync()
        ref = torch.zeros(Mw, N, device=DEV)
        for c in range(0, R, 65536):
            ref += dY[c:c + 65536].float().t() @ X[c:c + 65536].float()
        assert rel(out, ref) < 1e-4


def test_gemm_backward_data_bias_grad_big_tile():
    # fused bias-gradient column sums (dbias) of a bf16 backward-data epilogue, 256x256 tile
    M, N, K = 512, 512, 512
    torch.manual_seed(5)
    dY = torch.randn(M, K, device=DEV)
    W = torch.randn(K, N, device=DEV) * 0.1
    aux = torch.tanh(torch.randn(M, N, device=DEV))
    dYb, Wb, auxb = bf(dY), bf(W), bf(aux)
    o16 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    lib = ML.lib()
    # mmt_op_gemm has no dbias argument: reproduce the stored values and check the epilogue's
    # product, then the column sums through the model tests (test_gpu_model)
    rc = lib.mmt_op_gemm(_s(), 1, 0, ML.EPI["dtanh_bf16"], 1, M, N, K, ML.ptr(dYb), K, ML.ptr(Wb), N, None,
                         ML.ptr(auxb), N, None, 0, None, 0, ML.ptr(o16), N, 1.0)
    assert rc == 0
    _sync()
    ref = (dYb.float() @ Wb.float()) * (1 - auxb.float() ** 2)
    assert rel(o16, ref) < 1e-2


# --------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("R,C", [(1000, 256), (37, 32), (64, 512), (16, 1024), (9, 64)])
def test_layernorm(R, C):
    torch.manual_seed(R + C)
    x = torch.randn(R, C, device=DEV) * 3 + 1
    g = torch.randn(C, device=DEV)
    b = torch.randn(C, device=DEV)
    y = torch.empty(R, C, dtype=torch.bfloat16, device=DEV)
    mean = torch.empty(R, device=DEV)
    rstd = torch.empty(R, device=DEV)
    L = ML.lib()
    assert L.mmt_op_layernorm_fwd(_s(), R, C, ML.ptr(x), ML.ptr(g), ML.ptr(b), ML.ptr(y), ML.ptr(mean), ML.ptr(rstd)) == 0
    xr = x.clone().requires_grad_(True)
    gr = g.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-5)
    _sync()
    assert rel(y, ref) < 1e-2
    dy = torch.randn(R, C, device=DEV)
    ref.backward(dy)
    dx = torch.ones(R, C, device=DEV)
    dx16 = torch.empty(R, C, dtype=torch.bfloat16, device=DEV)
    dg = torch.zeros(C, device=DEV)
    db = torch.zeros(C, device=DEV)
    assert L.mmt_op_layernorm_bwd(_s(), R, C, ML.ptr(x), ML.ptr(g), ML.ptr(mean), ML.ptr(rstd), ML.ptr(dy), ML.ptr(dx),
                                  ML.ptr(dx16), ML.ptr(dg), ML.ptr(db)) == 0
    _sync()
    assert rel(dx - 1.0, xr.grad) < 1e-5
    assert rel(dx16, dx) < 1e-2
    assert rel(dg, gr.grad) < 1e-5
    assert rel(db, br.grad) < 1e-5


@pytest.mark.parametrize("M,N,K,drop", [(1000, 256, 1024, 0.0), (256, 256, 384, 0.1), (300, 256, 72, 0.1),
                                         (4096, 256, 256, 0.0), (2, 256, 450, 0.1), (1000, 512, 2048, 0.0),
                                         (300, 512, 768, 0.1), (130, 512, 72, 0.1),
                                         # every CU busy with the 128 x 512 tile's 3-stage ring (5 DMA
                                         # pieces per stage: the counted waits must be exact)
                                         (65536, 512, 2048, 0.0)])
def test_gemm_ln_bwd_fused(M, N, K, drop):
    """Backward-data GEMM with the LayerNorm backward fused into its epilogue (the engine's path at
    C = 256) against torch: dy = alpha A B in fp32, F.layer_norm's autograd for dx / dgamma / dbeta,
    the bf16 copy with the hash dropout mask of the consuming branch and its column sums."""
    import mmt_oracle as O
    torch.manual_seed(M + K)
    lda = r8(K)  # 16-B operand staging: row strides padded to 8 elements (as the engine's)
    A = pad_cols(bf(torch.randn(M, K, device=DEV)), lda)
    Bm = bf(torch.randn(K, N, device=DEV) * 0.05)
    x = torch.randn(M, N, device=DEV) * 2 + 0.5
    g = torch.randn(N, device=DEV)
    b = torch.randn(N, device=DEV)
    y = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    mean = torch.empty(M, device=DEV)
    rstd = torch.empty(M, device=DEV)
    L = ML.lib()
    assert L.mmt_op_layernorm_fwd(_s(), M, N, ML.ptr(x), ML.ptr(g), ML.ptr(b), ML.ptr(y), ML.ptr(mean), ML.ptr(rstd)) == 0
    alpha = 0.7
    dy = alpha * (A[:, :K].float() @ Bm.float())
    xr = x.clone().requires_grad_(True)
    gr = g.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (N,), gr, br, 1e-5).backward(dy)
    dx0 = torch.randn(M, N, device=DEV)
    dx = dx0.clone()
    dx16 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    dg = torch.zeros(N, device=DEV)
    db = torch.zeros(N, device=DEV)
    ds = torch.zeros(N, device=DEV)
    hd = O.HashDropout(7, drop) if drop else None
    key = 0x1234567
    assert L.mmt_op_gemm_ln_bwd(_s(), M, N, K, ML.ptr(A), lda, ML.ptr(Bm), N, alpha, ML.ptr(x), ML.ptr(g), ML.ptr(mean),
                                ML.ptr(rstd), ML.ptr(dx), ML.ptr(dx16), ML.ptr(dg), ML.ptr(db), ML.ptr(ds), key,
                                hd.thr if hd else 0, hd.scale if hd else 1.0) == 0
    _sync()
    assert rel(dx - dx0, xr.grad) < 1e-4
    assert rel(dg, gr.grad) < 1e-4
    assert rel(db, br.grad) < 1e-4
    if hd:
        rows = torch.arange(M).numpy()[:, None]
        cols = torch.arange(N).numpy()[None, :]
        exp16 = dx.cpu() * hd._mask(key, rows, cols)
    else:
        exp16 = dx.cpu()
    assert rel(dx16.cpu(), exp16) < 1e-2
    assert rel(ds.cpu(), exp16.sum(0)) < 1e-4
    # a row width other than 256 is refused, nothing launched
    assert L.mmt_op_gemm_ln_bwd(_s(), M, 128, K, ML.ptr(A), lda, ML.ptr(Bm), N, alpha, ML.ptr(x), ML.ptr(g), ML.ptr(mean),
                                ML.ptr(rstd), ML.ptr(dx), ML.ptr(dx16), ML.ptr(dg), ML.ptr(db), ML.ptr(ds), 0, 0,
                                1.0) == -2  # MMT_ERR_UNSUPPORTED


@pytest.mark.parametrize("bm", [128, 64])
@pytest.mark.parametrize("M,C,drop,lnf", [(1000, 256, 0.0, False), (300, 256, 0.1, True), (4096, 512, 0.1, False),
                                          (130, 512, 0.0, True), (65536, 512, 0.1, False), (65536, 256, 0.0, True),
                                          (97, 256, 0.1, False)])
def test_mlp2_fused(M, C, drop, lnf, bm):
    """The attention out-projection as one launch (mmt_op_mlp2: Linear(C, C/2) -> tanh -> Linear(C/2, C) ->
    hash dropout -> + residual, h kept in LDS; reference model.py:82-92) against torch on the same bf16
    operands: h (stored for the backward) within one bf16 rounding of the torch tanh, the fp32 output
    rel 1e-3 (h enters the second product as bf16 in both), the optional next LayerNorm on the owned
    rows; the full-chip cases keep every CU busy with both ring protocols. bm: rows per workgroup
    (mmt_mlp2_set_bm; 64 = the 4-wave form, C = 256 only: C = 512 keeps 128)."""
    old_bm = ML.lib().mmt_mlp2_set_bm(bm)
    try:
        _mlp2_fused_case(M, C, drop, lnf)
    finally:
        ML.lib().mmt_mlp2_set_bm(old_bm)


def _mlp2_fused_case(M, C, drop, lnf):
    import mmt_oracle as O
    torch.manual_seed(M + C)
    N1 = C // 2
    ldx = C
    x = bf(torch.randn(M, C, device=DEV))
    w0 = bf(torch.randn(N1, C, device=DEV) * 0.05)
    b0 = torch.randn(N1, device=DEV) * 0.1
    w2 = bf(torch.randn(C, N1, device=DEV) * 0.05)
    b2 = torch.randn(C, device=DEV) * 0.1
    resid = torch.randn(M, C, device=DEV)
    h = torch.zeros(M, N1, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(M, C, device=DEV)
    out16 = torch.zeros(M, C, dtype=torch.bfloat16, device=DEV)
    hd = O.HashDropout(11, drop) if drop else None
    key = 0x2468ACE
    g = torch.randn(C, device=DEV)
    be = torch.randn(C, device=DEV)
    ly = torch.zeros(M, C, dtype=torch.bfloat16, device=DEV) if lnf else None
    lm = torch.zeros(M, device=DEV) if lnf else None
    lr = torch.zeros(M, device=DEV) if lnf else None
    L = ML.lib()
    rc = L.mmt_op_mlp2(_s(), M, C, ML.ptr(x), ldx, ML.ptr(w0), C, ML.ptr(b0), ML.ptr(w2), N1, ML.ptr(b2), ML.ptr(h), N1,
                       ML.ptr(resid), ML.ptr(out), ML.ptr(out16), key, hd.thr if hd else 0, hd.scale if hd else 1.0,
                       ML.ptr(g) if lnf else None, ML.ptr(be) if lnf else None, ML.ptr(ly), ML.ptr(lm), ML.ptr(lr))
    assert rc == 0
    _sync()
    href = torch.tanh(x.float() @ w0.float().t() + b0)
    assert rel(h, href) < 8e-3
    y = h.float() @ w2.float().t() + b2  # the kernel's own bf16 h as the second operand
    if hd:
        rows = torch.arange(M).numpy()[:, None]
        cols = torch.arange(C).numpy()[None, :]
        y = y * hd._mask(key, rows, cols).to(DEV)
    ref = resid + y
    assert rel(out, ref) < 1e-4
    assert rel(out16, ref) < 1e-2
    if lnf:
        lref = torch.nn.functional.layer_norm(out, (C,), g, be, 1e-5)
        assert rel(ly, lref) < 1e-2
        assert rel(lm, out.mean(1)) < 1e-5
    # other widths are refused (the engine then runs the two GEMMs)
    assert L.mmt_op_mlp2(_s(), M, 128, ML.ptr(x), ldx, ML.ptr(w0), C, ML.ptr(b0), ML.ptr(w2), N1, ML.ptr(b2), ML.ptr(h),
                         N1, ML.ptr(resid), ML.ptr(out), None, 0, 0, 1.0, None, None, None, None, None) == -2


@pytest.mark.parametrize("M,C", [(1000, 256), (130, 512), (4096, 512), (65536, 512), (65536, 256)])
def test_mlp2_bwd_fused(M, C):
    """The out-projection's backward-data pair as one launch (mmt_op_mlp2_bwd) against torch on the same bf16
    operands: dh = (dy W2) * (1 - h^2) within one bf16 rounding, db0 its fp32 column sums, dx = dh W0 from the
    kernel's own bf16 dh (rel 1e-2: one more rounding)."""
    torch.manual_seed(M + C + 1)
    N1 = C // 2
    dy = bf(torch.randn(M, C, device=DEV))
    w2 = bf(torch.randn(C, N1, device=DEV) * 0.05)   # the forward's W2 [C][C/2]
    w0 = bf(torch.randn(N1, C, device=DEV) * 0.05)   # the forward's W0 [C/2][C]
    h = bf(torch.tanh(torch.randn(M, N1, device=DEV)))
    dh = torch.zeros(M, N1, dtype=torch.bfloat16, device=DEV)
    dx = torch.zeros(M, C, dtype=torch.bfloat16, device=DEV)
    db0 = torch.full((N1,), 0.5, device=DEV)
    alpha = 0.75
    L = ML.lib()
    rc = L.mmt_op_mlp2_bwd(_s(), M, C, ML.ptr(dy), C, ML.ptr(w2), N1, ML.ptr(h), N1, alpha, ML.ptr(w0), C, ML.ptr(dh),
                           N1, ML.ptr(db0), ML.ptr(dx))
    assert rc == 0
    _sync()
    dref = alpha * (dy.float() @ w2.float()) * (1 - h.float() ** 2)
    assert rel(dh, dref) < 1e-2
    assert rel(db0 - 0.5, dref.sum(0)) < 1e-4
    assert rel(dx, dh.float() @ w0.float()) < 1e-2


# --------------------------------------------------------------------------------- attention
def _attn_ref(q, ks, vs, scale, masks=None):
    # q [B,H,T,hs], ks/vs list of [B,H,T,hs]; sum over streams of causal softmax attention
    # masks (optional): per stream the scaled dropout mask [B,H,T,T] of the probabilities (keep / (1 - p))
    T = q.shape[2]
    mask = torch.tril(torch.ones(T, T, device=q.device)) == 0
    out = 0
    for j, (k, v) in enumerate(zip(ks, vs)):
        a = (q @ k.transpose(-1, -2)) * scale
        a = a.masked_fill(mask, float("-inf"))
        pr = torch.softmax(a, -1)
        if masks is not None:
            pr = pr * masks[j]
        out = out + pr @ v
    return out


@pytest.mark.parametrize("B,T,H,hs,ns", [(2, 64, 2, 32, 1), (3, 37, 4, 16, 1), (2, 4, 4, 8, 1), (2, 100, 2, 64, 1),
                                         (2, 64, 2, 32, 3), (1, 45, 3, 16, 2), (2, 256, 8, 32, 1), (1, 96, 2, 48, 2),
                                         # longer than one LDS chunk (256 rows at hs <= 32, 128 above)
                                         (1, 300, 2, 32, 1), (1, 300, 2, 32, 3), (1, 520, 2, 64, 2),
                                         (1, 1024, 1, 64, 1), (1, 257, 1, 24, 1)])
def test_attention_fwd_bwd(B, T, H, hs, ns, scratch=False, drop=0.0):
    """drop > 0 (test_attention_fwd_bwd_dropout): the same comparison under dropout of the probabilities, the keep
    bits from mmt_op_attention_mask, the reference with the scaled hash mask of tests/attn_drop_ref.py."""
    torch.manual_seed(B * 1000 + T * 10 + hs + ns)
    C = H * hs
    R = B * T
    # self-attention layout: q/k/v interleaved in one [R, 3C] buffer (engine layout) when ns == 1,
    # cross-attention layout: q [R, C], per-stream kv [R, 2C] with per-head [K|V] otherwise
    if ns == 1:
        qkv = bf(torch.randn(R, 3 * C, device=DEV))
        q, q_ld = qkv[:, C:2 * C], 3 * C
        ks, vs = [qkv[:, :C]], [qkv[:, 2 * C:]]
        kv_ld, kv_hs = 3 * C, hs
        kptr, vptr = [qkv], [qkv[:, 2 * C:]]
    else:
        qb = bf(torch.randn(R, C, device=DEV))
        q, q_ld = qb, C
        kvs = [bf(torch.randn(R, 2 * C, device=DEV)) for _ in range(ns)]
        ks = [kv.view(R, H, 2 * hs)[:, :, :hs].reshape(R, C) for kv in kvs]
        vs = [kv.view(R, H, 2 * hs)[:, :, hs:].reshape(R, C) for kv in kvs]
        kv_ld, kv_hs = 2 * C, 2 * hs
        kptr, vptr = kvs, [kv[:, hs:] for kv in kvs]

    def heads(x):
        return x.float().reshape(B, T, H, hs).permute(0, 2, 1, 3)

    scale = hs ** -0.5
    qf = heads(q).requires_grad_(True)
    kf = [heads(k).requires_grad_(True) for k in ks]
    vf = [heads(v).requires_grad_(True) for v in vs]
    L = ML.lib()
    masks, drop_args = None, ()
    if drop:
        import attn_drop_ref as DR
        key, thr, c = 0xD0D0 + T, DR.thr_of(drop), DR.scale_of(drop)
        masks = [torch.from_numpy(DR.keep_matrix(key, j, B, H, T, thr)).to(DEV).float() * c for j in range(ns)]
        nd = L.mmt_op_attention_mask_dwords(B, H, T)
        dmask = [torch.zeros(nd, dtype=torch.int32, device=DEV) for _ in range(ns)]
        mp = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in dmask])
        assert L.mmt_op_attention_mask(_s(), 1, B, T, H, (ctypes.c_int32 * 1)(ns), (ctypes.c_uint32 * 1)(key),
                                       (ctypes.c_uint32 * 1)(thr), mp) == 0
        drop_args = (key, thr, c, mp)
    ref = _attn_ref(qf, kf, vf, scale, masks)
    o = torch.zeros(R, C, dtype=torch.bfloat16, device=DEV)
    oj = [torch.zeros(R, C, dtype=torch.bfloat16, device=DEV) for _ in range(ns)]
    lse = [torch.zeros(B * H * T, device=DEV) for _ in range(ns)]
    kp = (ctypes.c_void_p * ns)(*[t.data_ptr() for t in kptr])
    vp = (ctypes.c_void_p * ns)(*[t.data_ptr() for t in vptr])
    fwd_args = (_s(), B, T, H, hs, ns, ML.ptr(q), q_ld, kp, vp, kv_ld, kv_hs, ML.ptr(o), C, ML.ptr_array(oj),
                ML.ptr_array(lse))
    rc = L.mmt_op_attention_fwd_drop(*fwd_args, *drop_args) if drop else L.mmt_op_attention_fwd(*fwd_args)
    assert rc == 0
    _sync()
    out = o.float().reshape(B, T, H, hs).permute(0, 2, 1, 3)
    assert rel(out, ref) < 1e-2, rel(out, ref)
    errs = [rel(out, ref)]
    if drop:  # lse is the unmasked softmax's, in the log2 domain: log2 sum_s 2^(log2(e) scale q.k_s)
        causal = torch.tril(torch.ones(T, T, device=DEV)) == 0
        for j in range(ns):
            a = (qf.detach().double() @ kf[j].detach().double().transpose(-1, -2)) * (scale * 1.4426950408889634)
            a = a.masked_fill(causal, float("-inf"))
            want = torch.log2(torch.exp2(a).sum(-1))
            got = lse[j].reshape(B, H, T).double()
            # relative 1e-5 of the row's magnitude. An lse, and a score itself, can cancel to near 0 while the
            # products it is summed from are O(1) (row 0 is one score): the fp32 dot product's error is relative to
            # sum_i |q_i k_i|, so the scale is the larger of |lse| and the row's largest sum_i |q_i k_i| (log2 domain)
            ab = (qf.detach().double().abs() @ kf[j].detach().double().abs().transpose(-1, -2)) * (scale * 1.4426950408889634)
            mag = torch.maximum(want.abs(), ab.masked_fill(causal, 0.0).amax(-1))
            ratio = (got - want).abs() / mag
            i = int(ratio.argmax())
            print(f"lse hs {hs} T {T} stream {j}: largest |error| / magnitude {ratio.flatten()[i].item():.3e} at row "
                  f"{i % T} (lse {want.flatten()[i].item():.6f}, got {got.flatten()[i].item():.6f}, "
                  f"largest sum |q k| {mag.flatten()[i].item():.3f})")
            assert (ratio <= 1e-5).all(), (j, ratio.max().item())
    # backward
    do = bf(torch.randn(R, C, device=DEV))
    ref.backward(heads(do))
    dq = torch.zeros(R, C, dtype=torch.bfloat16, device=DEV)
    if ns == 1:
        dqkv = torch.zeros(R, 3 * C, dtype=torch.bfloat16, device=DEV)
        dq_ptr, dq_ld = dqkv[:, C:], 3 * C
        dkp, dvp = [dqkv], [dqkv[:, 2 * C:]]
        dkv_ld, dkv_hs = 3 * C, hs
    else:
        dkvs = [torch.zeros(R, 2 * C, dtype=torch.bfloat16, device=DEV) for _ in range(ns)]
        dq_ptr, dq_ld = dq, C
        dkp, dvp = dkvs, [d[:, hs:] for d in dkvs]
        dkv_ld, dkv_hs = 2 * C, 2 * hs
    dvec = [torch.zeros(B * H * T, device=DEV) for _ in range(ns)]
    args = [_s(), B, T, H, hs, ns, ML.ptr(q), q_ld, kp, vp, kv_ld, kv_hs, ML.ptr(o), C, ML.ptr_array(oj),
            ML.ptr_array(lse), ML.ptr(do), C, ML.ptr_array(dvec), ML.ptr(dq_ptr), dq_ld,
            (ctypes.c_void_p * ns)(*[t.data_ptr() for t in dkp]), (ctypes.c_void_p * ns)(*[t.data_ptr() for t in dvp]),
            dkv_ld, dkv_hs]
    if scratch:  # fp32 dQ rows for the one-pass hs-32 backward over several KV streams (poisoned: fully written)
        dq32 = torch.full((R, C + 4), float("nan"), device=DEV)
        ws = (ML.ptr(dq32), C + 4)
    else:
        ws = (None, 0)
    if drop:
        rc = L.mmt_op_attention_bwd_drop(*args, *ws, *drop_args)
    elif scratch:
        rc = L.mmt_op_attention_bwd_ws(*args, *ws)
    else:
        rc = L.mmt_op_attention_bwd(*args)
    assert rc == 0
    _sync()
    if ns == 1:
        got_q = dqkv[:, C:2 * C]
        got_k = [dqkv[:, :C]]
        got_v = [dqkv[:, 2 * C:]]
    else:
        got_q = dq
        got_k = [d.view(R, H, 2 * hs)[:, :, :hs].reshape(R, C) for d in dkvs]
        got_v = [d.view(R, H, 2 * hs)[:, :, hs:].reshape(R, C) for d in dkvs]
    assert rel(heads(got_q), qf.grad) < 2e-2, rel(heads(got_q), qf.grad)
    for j in range(ns):
        assert rel(heads(got_k[j]), kf[j].grad) < 2e-2, (j, rel(heads(got_k[j]), kf[j].grad))
        assert rel(heads(got_v[j]), vf[j].grad) < 2e-2, (j, rel(heads(got_v[j]), vf[j].grad))
    if not drop:
        return
    # the masks act: the unmasked reference is more than 3x the achieved error away, in every output
    errs += [rel(heads(got_q), qf.grad)]
    errs += [rel(heads(got_k[j]), kf[j].grad) for j in range(ns)] + [rel(heads(got_v[j]), vf[j].grad) for j in range(ns)]
    masked = [ref.detach(), qf.grad] + [k.grad for k in kf] + [v.grad for v in vf]
    q0 = qf.detach().clone().requires_grad_(True)
    k0 = [k.detach().clone().requires_grad_(True) for k in kf]
    v0 = [v.detach().clone().requires_grad_(True) for v in vf]
    plain = _attn_ref(q0, k0, v0, scale)
    plain.backward(heads(do))
    unmasked = [plain.detach(), q0.grad] + [k.grad for k in k0] + [v.grad for v in v0]
    for e, a, b in zip(errs, masked, unmasked):
        assert rel(b, a) > 3 * e, (rel(b, a), e)


# one T per kernel path of tests/test_gpu_attn_dropout.py's table (the larger): (ring, hs, T, streams, scratch)
DROP_PATHS = AP.DROP_PATHS


@pytest.mark.parametrize("ring,hs,T,ns,scratch", DROP_PATHS)
def test_attention_fwd_bwd_dropout(ring, hs, T, ns, scratch):
    """Random N(0, 1) inputs under dropout (p = 0.1) through every attention kernel family, all three gradients:
    the read-outs of test_gpu_attn_dropout.py leave dK at zero and P uniform. The tolerances are
    test_attention_fwd_bwd's; also lse, which dropout must not change."""
    L = ML.lib()
    old = L.mmt_attn_set_ring(ring)
    try:
        test_attention_fwd_bwd(2, T, 3, hs, ns, scratch, drop=0.1)
    finally:
        L.mmt_attn_set_ring(old)


@pytest.mark.parametrize("ring", AP.HS64_RINGS)
@pytest.mark.parametrize("B,T,H,ns", AP.HS64_SHAPES)
def test_attention_hs64_backward_variants(B, T, H, ns, ring):
    """Every hs-64 attention variant (mmt_attn_set_ring: 0 the chunked dQ and dK/dV passes, 1 the
    slice-streamed dK/dV ring, 3 both rings with two query tiles per wave in the dQ ring, 7 that with
    the dK/dV ring at 3 waves per SIMD; bit 3 the slice-streamed forward: 8 with the chunked
    backward, 15 everything on the rings; bit 5 the one-pass backward where T <= 512 and one KV
    stream: 47) against the same torch reference, ragged T and multi-stream (up to 7 KV streams)
    included."""
    L = ML.lib()
    old = L.mmt_attn_set_ring(ring)
    try:
        # the launches below take the variant's kernels (the plan: host arithmetic, no launch)
        fwd, bwd, occ = AP.hs64_claim(ring, T, ns)
        assert AP.families(L, AP.kernel_test_call(AP.FWD, B, T, H, 64, ns)) == fwd
        got = AP.plan(L, AP.kernel_test_call(AP.BWD, B, T, H, 64, ns))
        assert tuple(l[0] for l in got) == bwd and (not occ or got[1][1][1] == occ)
        test_attention_fwd_bwd(B, T, H, 64, ns)
    finally:
        L.mmt_attn_set_ring(old)


@pytest.mark.parametrize("ring", AP.HS32_RINGS)
@pytest.mark.parametrize("B,T,H,ns,scratch", AP.HS32_SHAPES)
def test_attention_hs32_backward_variants(B, T, H, ns, scratch, ring):
    """The one-pass hs-32 backward (mmt_attn_set_ring bit 6, default: T <= 256; with bit 7 also several KV
    streams when the caller passes fp32 dQ scratch, mmt_op_attention_bwd_ws) and the two-pass pair (ring 15) against the
    same torch reference: full, ragged, two-position and one-tile sequences, up to 7 KV streams; without
    scratch the multi-stream cases, and every T > 256 case, take the two-pass pair under either knob."""
    L = ML.lib()
    old = L.mmt_attn_set_ring(ring)
    try:
        # the one-pass kernel where the docstring says so, the two-pass pair elsewhere (the plan: no launch)
        assert AP.families(L, AP.kernel_test_call(AP.BWD, B, T, H, 32, ns, scratch)) == AP.hs32_claim(ring, T, ns, scratch)
        test_attention_fwd_bwd(B, T, H, 32, ns, scratch)
    finally:
        L.mmt_attn_set_ring(old)


# ------------------------------------------------------------------------------ small kernels
@pytest.mark.parametrize("coal", [3, 0])
@pytest.mark.parametrize("R,H,hs", [(1000, 8, 32), (77, 4, 16), (300, 2, 64), (50, 4, 8), (5000, 8, 32),
                                    (3000, 16, 64), (33, 2, 64), (1055, 3, 32)])
def test_qkv2(R, H, hs, coal):
    """Per-head stage 2 forward / backward vs torch; the last shapes span several row blocks of
    the hs 32 / 64 backward (1024 rows each: dW2 partials added by atomics) with a ragged tail, or
    end one row into a 32-row tile. coal: the backward's row-slice loads through LDS (3: at hs
    32 and 64; the engine's default takes them at hs 64) or loads in the MFMA fragment layout (0)."""
    L0 = ML.lib()
    old = L0.mmt_qkv2_set_coal(coal)
    try:
        _qkv2(R, H, hs)
    finally:
        L0.mmt_qkv2_set_coal(old)


def _qkv2(R, H, hs):
    torch.manual_seed(R + H + hs)
    nblk, hh = 3 * H, hs // 2
    ld_h1, ld_out = r8(nblk * hh), nblk * hs
    h1 = torch.tanh(torch.randn(R, nblk * hh, device=DEV))
    h1b = bf(pad_cols(h1, ld_h1))
    w2 = torch.randn(nblk, hs, hh, device=DEV) * 0.2
    out = torch.zeros(R, ld_out, dtype=torch.bfloat16, device=DEV)
    L = ML.lib()
    assert L.mmt_op_qkv2_fwd(_s(), R, nblk, hs, ML.ptr(h1b), ld_h1, ML.ptr(w2), ML.ptr(out), ld_out) == 0
    hin = h1b.float()[:, : nblk * hh].view(R, nblk, hh).requires_grad_(True)
    wr = w2.clone().requires_grad_(True)
    ref = torch.einsum("rbi,boi->rbo", hin, wr)
    _sync()
    assert rel(out.view(R, nblk, hs), ref) < 1e-2
    dout = bf(torch.randn(R, ld_out, device=DEV))
    dh1 = torch.zeros(R, ld_h1, dtype=torch.bfloat16, device=DEV)
    dw2 = torch.zeros_like(w2)
    assert L.mmt_op_qkv2_bwd(_s(), R, nblk, hs, ML.ptr(h1b), ld_h1, ML.ptr(w2), ML.ptr(dout), ld_out, ML.ptr(dh1),
                             ML.ptr(dw2)) == 0
    ref.backward(dout.float().view(R, nblk, hs))
    _sync()
    hv = hin.detach()
    assert rel(dh1[:, : nblk * hh].view(R, nblk, hh), hin.grad * (1 - hv * hv)) < 1e-2
    assert rel(dw2, wr.grad) < 1e-4


@pytest.mark.parametrize("M,H,hs,K", [(1000, 8, 32, 256), (300, 2, 64, 72), (512, 8, 64, 1024), (77, 1, 32, 48),
                                     (16384 // 32, 8, 64, 512)])
def test_gemm_qkv_fused(M, H, hs, K):
    """Q/K/V stage 1 GEMM with the per-head stage 2 fused into its epilogue (mmt_op_gemm_qkv; the
    engine's forward at hs 32 / 64) against torch: h1 = tanh(X W1^T + b1), out = block-diagonal
    [hs/2 -> hs] maps of bf16(h1); a partial last column block (N = 48) and ragged rows. Shapes that
    take the 256 x 256 tile (M, N >= 256, K >= 1024) are refused with MMT_ERR_UNSUPPORTED (the
    engine then launches stage 2 as its own kernel)."""
    torch.manual_seed(M + H + hs + K)
    hh = hs // 2
    N = 3 * H * hh
    lda = r8(K)
    X = torch.randn(M, K, device=DEV)
    W1 = torch.randn(N, K, device=DEV) / K ** 0.5
    b1 = torch.randn(N, device=DEV) * 0.3
    w2 = torch.randn(N // hh, hs, hh, device=DEV) * 0.2
    Xb, Wb = bf(pad_cols(X, lda)), bf(pad_cols(W1, lda))
    ldh1, ldo = r8(N), 2 * N
    h1 = torch.zeros(M, ldh1, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(M, ldo, dtype=torch.bfloat16, device=DEV)
    L = ML.lib()
    rc = L.mmt_op_gemm_qkv(_s(), M, N, K, ML.ptr(Xb), lda, ML.ptr(Wb), lda, ML.ptr(b1), ML.ptr(h1), ldh1, ML.ptr(w2),
                           hh, ML.ptr(out), ldo)
    if M >= 256 and N >= 256 and K >= 1024:
        assert rc == -2  # MMT_ERR_UNSUPPORTED: the 256 x 256 tile has no fused stage 2
        return
    assert rc == 0
    _sync()
    ref_h1 = torch.tanh(Xb.float()[:, :K] @ Wb.float()[:, :K].t() + b1)
    assert rel(h1[:, :N], ref_h1) < 1e-2
    assert (h1[:, N:] == 0).all()  # pad columns of the next GEMM's operand stay zero
    ref = torch.einsum("rbi,boi->rbo", h1.float()[:, :N].view(M, N // hh, hh), bf(w2).float())
    assert rel(out.view(M, N // hh, hs), ref) < 1e-2
    # head sizes whose stage-1 block is not 16 / 32 columns are refused (the engine keeps qkv2_fwd)
    if hs == 32:
        assert L.mmt_op_gemm_qkv(_s(), M, 3 * H * 8, K, ML.ptr(Xb), lda, ML.ptr(Wb), lda, ML.ptr(b1), ML.ptr(h1), ldh1,
                                 ML.ptr(w2), 8, ML.ptr(out), ldo) == -2


@pytest.mark.parametrize("R,N,ld", [(16384, 1024, 1024), (1000, 450, 456), (77, 13, 16), (300, 6, 8)])
def test_colsum(R, N, ld):
    x = bf(torch.randn(R, ld, device=DEV))
    out = torch.full((N,), 2.0, device=DEV)
    assert ML.lib().mmt_op_colsum(_s(), R, N, ML.ptr(x), ld, ML.ptr(out), 0.5) == 0
    _sync()
    assert rel(out - 2.0, 0.5 * x.float()[:, :N].sum(0)) < 1e-5


@pytest.mark.parametrize("R,V", [(1000, 900), (77, 13), (64, 2), (33, 1), (500, 144), (20000, 900), (4097, 5), (9000, 1500)])
def test_cross_entropy(R, V):
    """Loss and dlogits against torch; R > 2048 makes every wave walk several rows (the next row's
    loads in flight, ragged last rows), V = 1500 takes the three-pass form."""
    torch.manual_seed(R + V)
    logits = torch.randn(R, V, device=DEV) * 2
    tgt = torch.randint(0, V, (R,), device=DEV)
    ld = r8(V)
    dl = torch.full((R, ld), 7.0, dtype=torch.bfloat16, device=DEV)
    loss = torch.zeros(1, device=DEV)
    assert ML.lib().mmt_op_cross_entropy(_s(), R, V, ML.ptr(logits), ML.ptr(tgt), ML.ptr(dl), ld, ML.ptr(loss)) == 0
    lr = logits.clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lr, tgt)
    ref.backward()
    _sync()
    torch.testing.assert_close(loss[0], ref.detach(), rtol=1e-5, atol=1e-5)
    assert rel(dl[:, :V].float() / R, lr.grad) < 1e-2
    assert (dl[:, V:].float() == 0).all()


@pytest.mark.parametrize("B,T,C,V", [(4, 32, 64, 57), (2, 256, 256, 900), (3, 4, 32, 3), (4, 256, 256, 3000), (2, 64, 64, 5000)])
def test_embedding(B, T, C, V):
    torch.manual_seed(B + T + C + V)
    idx = torch.randint(0, V, (B, T), device=DEV)
    tok = torch.randn(V, C, device=DEV)
    pos = torch.randn(T, C, device=DEV)
    x = torch.empty(B * T, C, device=DEV)
    L = ML.lib()
    assert L.mmt_op_embedding_fwd(_s(), B, T, C, V, ML.ptr(idx), ML.ptr(tok), ML.ptr(pos), ML.ptr(x)) == 0
    _sync()
    torch.testing.assert_close(x.view(B, T, C), tok[idx] + pos[None])
    dx = torch.randn(B * T, C, device=DEV)
    dtok = torch.zeros(V, C, device=DEV)
    dpos = torch.zeros(T, C, device=DEV)
    assert L.mmt_op_embedding_bwd(_s(), B, T, C, V, ML.ptr(idx), ML.ptr(dx), ML.ptr(dtok), ML.ptr(dpos)) == 0
    _sync()
    ref_tok = torch.zeros(V, C, device=DEV).index_add_(0, idx.view(-1), dx)
    torch.testing.assert_close(dtok, ref_tok, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dpos, dx.view(B, T, C).sum(0), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("sort", [1, 0])
@pytest.mark.parametrize("B,T,C,V", [(2, 256, 256, 900), (64, 256, 256, 900), (16, 1024, 512, 5), (64, 256, 256, 13),
                                     (8, 512, 256, 144), (3, 4, 32, 3), (1, 64, 64, 200), (4, 256, 1024, 900),
                                     (2, 96, 64, 5000), (1, 100, 96, 16384), (2, 33, 40, 7)])
def test_embedding_bwd_scratch(B, T, C, V, sort):
    """Token-table gradient of the scratch path (mmt_op_embedding_bwd_ws: the engine's) against torch
    index_add, accumulating into a non-zero dtok. sort=1 (default): counting sort of the rows by token
    + per-run sums (incl. the largest vocabulary the histogram holds, ragged row counts and column
    widths); sort=0: the LDS-privatised slabs with per-chunk partial tables ((1, 64, 64, 200): the
    tables do not fit B*T*C floats, so the atomic flush runs; (2, 96, 64, 5000): a table too large
    for a 4-float LDS slab takes direct atomics)."""
    L0 = ML.lib()
    old = L0.mmt_emb_set_sort(sort)
    try:
        _embedding_bwd_scratch(B, T, C, V)
    finally:
        L0.mmt_emb_set_sort(old)


def _embedding_bwd_scratch(B, T, C, V):
    torch.manual_seed(B + T + C + V)
    idx = torch.randint(0, V, (B, T), device=DEV)
    dx = torch.randn(B * T, C, device=DEV)
    dtok0 = torch.randn(V, C, device=DEV)
    dtok = dtok0.clone()
    dpos = torch.zeros(T, C, device=DEV)
    scratch = torch.full((B * T * C,), float("nan"), device=DEV)
    L = ML.lib()
    assert L.mmt_op_embedding_bwd_ws(_s(), B, T, C, V, ML.ptr(idx), ML.ptr(dx), ML.ptr(dtok), ML.ptr(dpos),
                                     ML.ptr(scratch)) == 0
    _sync()
    ref_tok = dtok0.clone().index_add_(0, idx.view(-1), dx)
    torch.testing.assert_close(dtok, ref_tok, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(dpos, dx.view(B, T, C).sum(0), rtol=1e-5, atol=1e-4)

