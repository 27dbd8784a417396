"""Exact inputs and references for the linear kernel family (tests/test_gpu_exact_kernels.py).

Every kernel whose arithmetic is only multiply, add, max, select and bf16 rounding has inputs on which every
intermediate is exactly representable in fp32: small integers, halves and quarters, a power-of-two alpha. On such
inputs the result does not depend on the accumulation order, split-K, the order of atomics or the tile shape, so
the correct answer is ONE bit pattern per element and the comparison needs no tolerance.

The sufficient condition (assert_exact): with every input a multiple of some step and `unit` the product of the
steps that meet in one output element, every partial sum of any subset of the terms is a multiple of `unit` and
its magnitude is at most sum_k |a||b| |alpha| + |bias| + |resid| + |prefill|. Below 2^24 units all of those are
fp32 numbers (24-bit significand), so no addition in any order rounds.

The references are fp64 (exact for these ranges; f32_exact checks that the value is an fp32 number) and round to
bf16 only where the kernel documents a bf16 store: the FFN's h, mlp2_bwd's dh, stage 2's bf16(W2).

Plain torch / numpy on the CPU, no GPU.
"""
import functools

import numpy as np
import torch

LIMIT = float(1 << 24)


def r8(x):
    """Leading dimension of a bf16 GEMM operand: a multiple of 8 elements (16-byte staging), at least 8."""
    return max(8, (x + 7) // 8 * 8)


def r4(x):
    return (x + 3) // 4 * 4


# ------------------------------------------------------------------------------------------ generators
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def bf16_exact(t):
    return torch.equal(t.float().to(torch.bfloat16).float(), t.float())


def ints(shape, lo, hi, seed, step=1.0, bf16=True):
    """Uniform multiples of `step` in [lo, hi] as fp32 (step 1: integers, 0.5: halves, 0.25: quarters). bf16: the
    tensor is stored as bf16 by its test, so every value must be a bf16 number (fp32 operands pass False)."""
    klo, khi = int(round(lo / step)), int(round(hi / step))
    t = torch.randint(klo, khi + 1, tuple(shape), generator=_gen(seed)).float() * step
    assert not bf16 or bf16_exact(t), (lo, hi, step)
    return t


def choice(shape, values, seed):
    """Uniform draws from `values` (bf16-exact numbers) as fp32."""
    v = torch.tensor(values, dtype=torch.float32)
    assert bf16_exact(v), values
    return v[torch.randint(0, len(values), tuple(shape), generator=_gen(seed))]


def signed_zeros(t, seed):
    """Half of the zeros of t become -0.0 (bf16 0x8000): ReLU' must treat both as not positive."""
    flip = torch.rand(t.shape, generator=_gen(seed)) < 0.5
    return torch.where((t == 0) & flip, torch.full_like(t, -0.0), t)


def pad_cols(t, ld, fill=0.0):
    """t [rows, n] in a [rows, ld] buffer, the pad columns holding `fill`."""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, : t.shape[1]] = t
    return out


# --------------------------------------------------------------------------------------------- rounding
def f32_exact(x64):
    """fp64 -> fp32 of a value that must be an fp32 number already (else the reference would round twice)."""
    x64 = torch.as_tensor(x64, dtype=torch.float64)
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), "reference value is not an fp32 number"
    return x32


def rne_bf16(x):
    """fp32 -> bf16, round to nearest even (torch's conversion). fp64 input must be an fp32 number."""
    x = torch.as_tensor(x)
    if x.dtype == torch.float64:
        x = f32_exact(x)
    return x.float().to(torch.bfloat16)


# ------------------------------------------------------------------------------------- order independence
def assert_exact(a_abs, b_abs, extra=0.0, alpha=1.0, unit=1.0):
    """The sufficient condition for order independence of alpha * a @ b + extra, for every output element:
    sum_k |a||b| |alpha| + extra < 2^24 units. a_abs [M, K] and b_abs [K, N] are |inputs| (or per-column / per-row
    maxima of them: any upper bound), extra = |bias| + |resid| + |prefill| broadcastable to [M, N], unit the
    smallest step any intermediate takes (1 for integers; the product of the steps when halves or quarters and a
    fractional alpha are present). Returns the largest bound in units."""
    a = torch.as_tensor(a_abs, dtype=torch.float64).abs()
    b = torch.as_tensor(b_abs, dtype=torch.float64).abs()
    bound = (a @ b) * abs(alpha) + torch.as_tensor(extra, dtype=torch.float64).abs()
    worst = float(bound.max()) / unit if bound.numel() else 0.0
    assert worst < LIMIT, f"inputs are not order independent: bound {worst:.0f} units >= 2^24"
    # the terms are multiples of the unit: the distinct |a| x |b| products and the extra term
    ua, ub = torch.unique(a)[:256], torch.unique(b)[:256]
    for t in (ua[:, None] * ub[None, :] * abs(alpha) / unit, torch.as_tensor(extra, dtype=torch.float64) / unit):
        assert torch.equal(t, t.round()), "a term is not a multiple of the unit"
    return worst


# -------------------------------------------------------------------------------------------- references
def gemm64(a, b_kn, alpha=1.0, bias=None, add=None):
    """alpha * a[M, K] @ b[K, N] + bias[N] + add[M, N] in fp64."""
    v = alpha * (a.double() @ b_kn.double())
    if bias is not None:
        v = v + bias.double()
    if add is not None:
        v = v + add.double()
    return v


def epilogue(epi, v64, aux=None):
    """The stored value of mmt_op_gemm's exact epilogues from the fp64 pre-activation value v64 (alpha, bias,
    residual / prefill already in). aux: the bf16 aux operand's values."""
    if epi in ("store_f32", "bias_resid_f32", "acc_f32", "atomic_f32"):
        return f32_exact(v64)
    if epi == "store_bf16":
        return rne_bf16(v64)
    if epi == "bias_relu_bf16":
        return rne_bf16(v64.clamp(min=0.0))
    if epi == "drelu_bf16":  # keeps the value iff aux > 0 (+0 and -0 are not)
        return rne_bf16(torch.where(aux.double() > 0, v64, torch.zeros_like(v64)))
    if epi == "dtanh_bf16":
        return rne_bf16(v64 * (1.0 - aux.double() ** 2))
    raise ValueError(epi)


def ffn_ref(x, w0, b0, w2, b2, resid):
    """mmt_op_ffn without dropout: h = RNE(relu(x W0^T + b0)) (the documented bf16 store), out = resid + h16 W2^T
    + b2 (fp32, exact), out16 = RNE(out)."""
    h = rne_bf16(gemm64(x, w0.t(), bias=b0).clamp(min=0.0))
    out = f32_exact(gemm64(h.float(), w2.t(), bias=b2, add=resid))
    return h, out, out.to(torch.bfloat16)


def mlp2_bwd_ref(dy, w2, h, alpha, w0):
    """mmt_op_mlp2_bwd: d = alpha (dy W2) (1 - h^2) in fp32; dh = RNE(d) (the documented bf16 store); db0 = the
    column sums of d BEFORE that store (mlp2_bwd_kernel sums its fp32 registers); dx = RNE(dh16 W0)."""
    d = gemm64(dy, w2, alpha=alpha) * (1.0 - h.double() ** 2)
    dh = rne_bf16(d)
    db0 = f32_exact(d.sum(0))
    dx = rne_bf16(gemm64(dh.float(), w0))
    return dh, db0, dx, d


def mlp2_bwd_db0_of_stored(dh):
    """The other convention (column sums of the STORED bf16 dh), to show that the inputs tell the two apart."""
    return dh.double().sum(0)


def qkv2_fwd_ref(h1, w2):
    """out[r, blk, o] = RNE(sum_i bf16(W2)[blk, o, i] h1[r, blk, i]); h1 [R, nblk, hh], w2 [nblk, hs, hh]."""
    w = rne_bf16(w2).double()
    return rne_bf16(torch.einsum("rbi,boi->rbo", h1.double(), w))


def qkv2_bwd_ref(h1, w2, dout, dw2_prefill):
    """dh1 = RNE((dout bf16(W2)) (1 - h1^2)), dw2 = prefill + sum_r dout[r, blk, o] h1[r, blk, i] (fp32, exact)."""
    w = rne_bf16(w2).double()
    g = torch.einsum("rbo,boi->rbi", dout.double(), w)
    dh1 = rne_bf16(g * (1.0 - h1.double() ** 2))
    dw2 = f32_exact(dw2_prefill.double() + torch.einsum("rbo,rbi->boi", dout.double(), h1.double()))
    return dh1, dw2


def e4m3_bytes(t):
    """e4m3fn bytes of small integers (exact in e4m3: |v| <= 16)."""
    q = t.to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), t.float())
    return q.view(torch.uint8)


def e8m0_bytes(rows, nblocks, lds, seed):
    """Hand-set E8M0 exponent bytes from {126, 127, 128} (scales 0.5, 1, 2), a different one per row and per
    32-column block; the pad bytes hold 127. Returns (bytes [rows, lds] uint8, scales [rows, nblocks] fp64)."""
    e = torch.randint(126, 129, (rows, nblocks), generator=_gen(seed))
    b = torch.full((rows, lds), 127, dtype=torch.uint8)
    b[:, :nblocks] = e.to(torch.uint8)
    return b, torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 127).double())


def mx_dequant64(vals, scales):
    """vals [rows, K] * scales [rows, K / 32] per 32-column block, fp64."""
    r, k = vals.shape
    return (vals.double().view(r, k // 32, 32) * scales.unsqueeze(-1)).view(r, k)


# ----------------------------------------------------------------------------------------------- report
def report_mismatch(got, want, what=""):
    """A message for a failed bit-exact comparison of two [rows, cols] tensors: the count of differing elements,
    the first 8 as (row, col, got, want), and the sets of rows mod 32 / columns mod 8 they fall in (a whole tile,
    an edge group and a rounding problem look different there)."""
    g = torch.as_tensor(got).detach().cpu()
    w = torch.as_tensor(want).detach().cpu()
    if g.shape != w.shape:
        return f"{what}: shape {tuple(g.shape)} != {tuple(w.shape)}"
    g2 = g.reshape(-1, g.shape[-1]) if g.dim() > 1 else g.reshape(1, -1)
    w2 = w.reshape(g2.shape)
    bad = (g2.double() != w2.double()) | (torch.isnan(g2.double()) | torch.isnan(w2.double()))
    n = int(bad.sum())
    if n == 0:
        return f"{what}: no differing element"
    idx = bad.nonzero()
    first = [(int(r), int(c), float(g2[r, c]), float(w2[r, c])) for r, c in idx[:8].tolist()]
    rows = sorted({int(r) % 32 for r in idx[:, 0].tolist()})
    cols = sorted({int(c) % 8 for c in idx[:, 1].tolist()})
    return (f"{what}: {n} of {bad.numel()} elements differ; first (row, col, got, want): {first}; "
            f"rows mod 32: {rows}; cols mod 8: {cols}")


def sums_in_random_orders(a, b_kn, rows, cols, seeds=(1, 2, 3)):
    """The fp32 sums of the products a[m, k] b[k, n] for m in rows, n in cols, accumulated serially in numpy float32
    in len(seeds) random orders of k: a list of [len(rows), len(cols)] float32 arrays."""
    an = a[rows].numpy().astype(np.float32)
    bn = b_kn[:, cols].numpy().astype(np.float32)
    prod = an[:, None, :] * bn.T[None, :, :]  # [rows, cols, K], each product exact
    out = []
    for s in seeds:
        perm = np.random.RandomState(s).permutation(prod.shape[-1])
        out.append(np.cumsum(prod[..., perm], axis=-1, dtype=np.float32)[..., -1])
    return out


# ------------------------------------------------------------------------------------------ input sets
# The inputs of tests/test_gpu_exact_kernels.py, made once per shape and never modified (functools.lru_cache), each
# checked with assert_exact where it is made: an input set that could differ by accumulation order fails here, on
# the CPU, not as a kernel mismatch. tests/test_exact_ref_cpu.py builds every one at the largest shape.

# K-tiles of BK 32 / BK 64: 32 -> 1 / 1, 45 -> 2 / 1, 72 and 96 -> 3 / 2, 164 -> 6 / 3 (ragged: 164 % 8 = 4), 256 -> 8 / 4,
# 512 and up: many
GEMM_SHAPES = [(33, 17, 45), (200, 136, 72), (128, 450, 256), (5, 264, 96), (256, 256, 32), (300, 264, 520),
               (512, 256, 512), (520, 328, 1032), (130, 72, 164)]
WGRAD_SHAPES = [(450, 256, 3000), (6, 32, 300), (384, 256, 4096), (33, 45, 77)]
BWD_ALPHAS = (1.0, 0.5)
ATOMIC_ALPHA = 0.25


@functools.lru_cache(maxsize=None)
def gemm_fwd_case(M, N, K):
    """Forward (a_kc = 1, b_kc = 1): X in [-4, 4], W in [-3, 3], integer bias and residual. From K = 64 on many
    results pass 256, where every odd integer is a bf16 tie: the rounding mode is visible."""
    s = 1000 * M + 10 * N + K
    X, W = ints((M, K), -4, 4, s), ints((N, K), -3, 3, s + 1)
    bias, resid = ints((N,), -64, 64, s + 2), ints((M, N), -100, 100, s + 3)
    assert_exact(X.abs(), W.abs().t(), extra=bias.abs() + resid.abs())
    return dict(X=X, W=W, bias=bias, resid=resid, base=gemm64(X, W.t()))


def gemm_fwd_want(c, epi):
    """(o32, o16) of a forward epilogue (None: the buffer is not written). bias_resid_f32 also stores the bf16
    copy of its result when the caller passes o16 (GemmProblem::o16, the engine's LayerNorm-free residual rows)."""
    if epi == "store_bf16":
        return None, epilogue(epi, c["base"])
    v = c["base"] + c["bias"].double()
    if epi == "bias_relu_bf16":
        return None, epilogue(epi, v)
    if epi == "bias_resid_f32":
        o = epilogue(epi, v + c["resid"].double())
        return o, o.to(torch.bfloat16)
    return epilogue(epi, v), None


@functools.lru_cache(maxsize=None)
def gemm_bwd_case(M, N, K):
    """Backward-data (b_kc = 0): dX[M, N] = alpha dY[M, K] W[K, N]; ReLU' aux with positive and negative values,
    +0 and -0; tanh' aux in {0, +-0.5, +-1} (1 - a^2 in {1, 0.75, 0}); an integer prefill for acc_f32."""
    s = 2000 * M + 20 * N + K
    dY, W = ints((M, K), -4, 4, s), ints((K, N), -3, 3, s + 1)
    aux_relu = signed_zeros(ints((M, N), -2, 2, s + 2), s + 3)
    aux_tanh = choice((M, N), [0.0, 0.5, -0.5, 1.0, -1.0], s + 4)
    prefill = ints((M, N), -100, 100, s + 5)
    for alpha in BWD_ALPHAS:  # unit: alpha's half x tanh's quarter
        assert_exact(dY.abs(), W.abs(), extra=prefill.abs(), alpha=alpha, unit=0.125)
    return dict(dY=dY, W=W, aux_relu=aux_relu, aux_tanh=aux_tanh, prefill=prefill, base=gemm64(dY, W))


def gemm_bwd_want(c, epi, alpha):
    """(o32, o16) of a backward-data epilogue; acc_f32 also stores the bf16 copy of the accumulated value when the
    caller passes o16."""
    v = alpha * c["base"]
    if epi == "store_f32":
        return epilogue(epi, v), None
    if epi == "acc_f32":
        o = epilogue(epi, v + c["prefill"].double())
        return o, o.to(torch.bfloat16)
    aux = {"drelu_bf16": c["aux_relu"], "dtanh_bf16": c["aux_tanh"]}.get(epi)
    return None, epilogue(epi, v, aux)


@functools.lru_cache(maxsize=None)
def gemm_wgrad_case(M, N, R):
    """Weight gradient out[M, N] = prefill + 0.25 dY[R, M]^T X[R, N] (mmt_op_gemm atomic_f32 and mmt_op_gemm_wgrad)."""
    s = 3000 * M + 30 * N + R
    dY, X = ints((R, M), -4, 4, s), ints((R, N), -3, 3, s + 1)
    prefill = ints((M, N), -100, 100, s + 2)
    assert_exact(dY.abs().t(), X.abs(), extra=prefill.abs(), alpha=ATOMIC_ALPHA, unit=0.25)
    return dict(dY=dY, X=X, prefill=prefill, want=f32_exact(gemm64(dY.t(), X, alpha=ATOMIC_ALPHA, add=prefill)))


@functools.lru_cache(maxsize=None)
def colsum_case(R, N, ld):
    x = ints((R, N), -8, 8, 7 * R + N)
    prefill = ints((N,), -50, 50, 7 * R + N + 1)
    assert_exact(torch.ones(1, R), x.abs(), extra=prefill.abs(), alpha=0.5, unit=0.5)
    return dict(x=x, prefill=prefill, want=f32_exact(prefill.double() + 0.5 * x.double().sum(0)))


@functools.lru_cache(maxsize=None)
def ordered_sum_case(nparts, n):
    parts = ints((nparts, n), -1000, 1000, 11 * nparts + n, bf16=False)
    prefill = ints((n,), -50, 50, 11 * nparts + n + 1)
    assert_exact(torch.ones(1, nparts), parts.abs(), extra=prefill.abs())
    return dict(parts=parts, prefill=prefill, want=f32_exact(prefill.double() + parts.double().sum(0)))


QKV2_SHAPES = [(77, 4, 16), (50, 4, 8), (300, 2, 64), (1055, 3, 32), (33, 2, 64), (1100, 2, 64)]


@functools.lru_cache(maxsize=None)
def qkv2_case(R, H, hs):
    """Per-head stage 2: h1 in {0, +-0.5, +-1} (tanh' exact), integer W2 in [-4, 4] (bf16(W2) exact), integer dout
    in [-8, 8], integer dW2 prefill. dW2 sums R rows through atomics over 1024-row blocks: still one bit pattern."""
    nblk, hh = 3 * H, hs // 2
    s = 5000 * R + 50 * H + hs
    h1 = choice((R, nblk, hh), [0.0, 0.5, -0.5, 1.0, -1.0], s)
    w2 = ints((nblk, hs, hh), -4, 4, s + 1)
    dout = ints((R, nblk, hs), -8, 8, s + 2)
    pre = ints((nblk, hs, hh), -100, 100, s + 3)
    assert_exact(torch.ones(1, hh), torch.full((hh, 1), 4.0), unit=0.5)                       # forward
    assert_exact(torch.full((1, hs), 8.0), torch.full((hs, 1), 4.0), unit=0.25)               # dh1 (x tanh')
    assert_exact(torch.full((1, R), 8.0), torch.ones(R, 1), extra=100.0, unit=0.5)            # dW2
    out = qkv2_fwd_ref(h1, w2)
    dh1, dw2 = qkv2_bwd_ref(h1, w2, dout, pre)
    return dict(h1=h1, w2=w2, dout=dout, pre=pre, out=out, dh1=dh1, dw2=dw2)


MLP2_BWD_CASES = [(130, 256), (300, 256), (130, 512), (300, 512)]


@functools.lru_cache(maxsize=None)
def mlp2_bwd_case(M, C, alpha):
    """mmt_op_mlp2_bwd: h in {0, +-0.5, +-1}, integer dy in [-8, 8], W2 and W0 in {-1, 0, 1}, an integer db0
    prefill. d = alpha (dy W2) (1 - h^2) takes eighths (alpha 0.5 x 0.75), so RNE(d) != d in many places and the
    two db0 conventions (sums of d, sums of the stored dh) differ."""
    N1 = C // 2
    s = 7000 * M + C + int(alpha * 8)
    dy = ints((M, C), -8, 8, s)
    w2 = choice((C, N1), [-1.0, 0.0, 1.0], s + 1)
    w0 = choice((N1, C), [-1.0, 0.0, 1.0], s + 2)
    h = choice((M, N1), [0.0, 0.5, -0.5, 1.0, -1.0], s + 3)
    pre = ints((N1,), -50, 50, s + 4)
    assert_exact(dy.abs(), w2.abs(), alpha=alpha, unit=0.125)
    dh, db0, dx, d = mlp2_bwd_ref(dy, w2, h, alpha, w0)
    assert_exact(dh.float().abs(), w0.abs(), unit=0.125)                                # dx from the stored dh
    assert_exact(torch.ones(1, M), d.abs(), extra=pre.abs(), unit=0.125)                # db0
    return dict(dy=dy, w2=w2, w0=w0, h=h, pre=pre, dh=dh, dx=dx, d=d, db0=f32_exact(pre.double() + db0.double()),
                db0_stored=pre.double() + mlp2_bwd_db0_of_stored(dh))


FFN_C, FFN_HID = 256, 1024


@functools.lru_cache(maxsize=None)
def ffn_weights():
    """W0, W2 in {-1, 0, 1}; b0 in [-300, 300] lifts many hidden values past 256 (bf16 ties), integer b2."""
    return dict(w0=choice((FFN_HID, FFN_C), [-1.0, 0.0, 1.0], 41), b0=ints((FFN_HID,), -300, 300, 42, bf16=False),
                w2=choice((FFN_C, FFN_HID), [-1.0, 0.0, 1.0], 43), b2=ints((FFN_C,), -64, 64, 44))


@functools.lru_cache(maxsize=None)
def ffn_case(M, seed):
    w = ffn_weights()
    x = ints((M, FFN_C), -2, 2, seed)
    resid = ints((M, FFN_C), -100, 100, seed + 1)
    assert_exact(x.abs(), w["w0"].abs().t(), extra=w["b0"].abs())
    h, out, out16 = ffn_ref(x, w["w0"], w["b0"], w["w2"], w["b2"], resid)
    assert_exact(h.float().abs(), w["w2"].abs().t(), extra=w["b2"].abs() + resid.abs())
    return dict(x=x, resid=resid, h=h, out=out, out16=out16)


EMB_SHAPES = [(3, 4, 32, 3), (2, 33, 40, 7), (1, 64, 64, 200), (2, 96, 64, 5000), (2, 256, 256, 900)]


@functools.lru_cache(maxsize=None)
def embedding_case(B, T, C, V):
    s = B + 10 * T + 100 * C + V
    idx = torch.randint(0, V, (B, T), generator=_gen(s))
    tok, pos = ints((V, C), -50, 50, s + 1), ints((T, C), -50, 50, s + 2)
    dx = ints((B * T, C), -8, 8, s + 3)
    dtok0, dpos0 = ints((V, C), -100, 100, s + 4), ints((T, C), -100, 100, s + 5)
    assert_exact(torch.ones(1, B * T), dx.abs(), extra=100.0)  # every row into one token: the worst case
    return dict(idx=idx, tok=tok, pos=pos, dx=dx, dtok0=dtok0, dpos0=dpos0, x=f32_exact((tok[idx] + pos[None]).double()).view(B * T, C),
                dtok=f32_exact(dtok0.double().index_add_(0, idx.view(-1), dx.double())),
                dpos=f32_exact(dpos0.double() + dx.double().view(B, T, C).sum(0)))


F8_SHAPES = [(33, 64, 32), (300, 200, 96), (128, 264, 256), (200, 96, 128)]


@functools.lru_cache(maxsize=None)
def f8_case(M, N, K):
    """MX-fp8 GEMM: e4m3 bytes of integers in [-4, 4], hand-set E8M0 bytes from {126, 127, 128} per row and
    32-column block, integer bias. Products take quarters (0.5 x 0.5)."""
    s = 9000 * M + 90 * N + K
    a, b = ints((M, K), -4, 4, s), ints((N, K), -4, 4, s + 1)
    lds = (K // 32 + 3) // 4 * 4
    sa, sca = e8m0_bytes(M, K // 32, lds, s + 2)
    sb, scb = e8m0_bytes(N, K // 32, lds, s + 3)
    bias = ints((N,), -64, 64, s + 4)
    A, Bm = mx_dequant64(a, sca), mx_dequant64(b, scb)
    assert_exact(A.abs(), Bm.abs().t(), extra=bias.abs(), unit=0.25)
    v = f32_exact(gemm64(A, Bm.t(), bias=bias))
    return dict(a8=e4m3_bytes(a), b8=e4m3_bytes(b), sa=sa, sb=sb, lds=lds, bias=bias, v=v, relu=v.clamp(min=0.0))
