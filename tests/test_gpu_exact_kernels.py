"""The linear kernel family bit for bit (tests/exact_ref.py: exact inputs, fp64 references).

On small integers, halves and a power-of-two alpha every intermediate of these kernels is an fp32 number, so the
result is independent of accumulation order, split-K, atomics and tile shape: each test compares WHOLE outputs
with torch.equal, no tolerance. What the relative-norm tests cannot see shows here: a few wrong elements at a
ragged edge, a rounding mode other than round-to-nearest-even (results pass 256, where odd integers are bf16
ties), a pad column that is not zeroed, a write past the output.

Pads and guards (_Buf), as the kernels have them (mmt_gemm_dev.h epi_pad, issue_tile, the vector epilogue):
  * K-contiguous GEMM operands are staged in 8-element K chunks whose first index is tested against K, so their
    columns K..r8(K) are read and must be zero: they are zero here. Pad columns of MN-contiguous operands (the
    b_kc = 0 B, both weight-gradient operands) and of every other input only feed discarded outputs or are not
    read at all: they hold 1000.
  * every output lies between two guard bands of 256 elements and has pad columns, all prefilled with a sentinel.
    After the call the logical area equals the reference; for a bf16 GEMM output the columns N..min(r8(N), ld) of
    the rows < M are zero (the next GEMM reads them as K padding; the scalar edge epilogue writes them, up to the
    leading dimension); everything else still holds the sentinel. A stray write shows as a changed sentinel:
    nothing relies on a fault, nothing a kernel may read is NaN.
  * atomic_f32, acc_f32 and the += outputs: the logical area is prefilled with integers, part of the expected
    value.
"""
import contextlib
import ctypes
import functools

import pytest
import torch

import exact_ref as E
import mmt_lib as ML

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
SENT = {torch.bfloat16: -1000.0, torch.float32: -12345.0, torch.uint8: 0xA5}
PAD_IN = 1000.0  # pad columns of inputs that must not influence the result (a bf16 number)


def _s():
    return ML.stream_ptr()


class _Buf:
    """An output [rows, ld] (n logical columns) between two guard bands, everything prefilled with the sentinel
    of its type; `prefill` (CPU [rows, n]) goes into the logical area."""

    def __init__(self, rows, n, ld, dtype, prefill=None):
        assert ld >= n
        self.rows, self.n, self.ld, self.sent = rows, n, ld, SENT[dtype]
        self.flat = torch.full((2 * GUARD + rows * ld,), self.sent, dtype=dtype, device=DEV)
        self.t = self.flat[GUARD:GUARD + rows * ld].view(rows, ld)
        if prefill is not None:
            self.t[:, :n] = prefill.reshape(rows, n).to(DEV)

    def ptr(self):
        return ML.ptr(self.t)

    def check(self, want, what, zero_pad=False):
        """want (CPU, the buffer's dtype; None: the call must not write here) == the logical area; zero_pad: the
        pad columns N..r8(N) of a bf16 GEMM output are zero; all the rest is the sentinel."""
        t, z = self.t, 0
        if want is not None:
            w = want.reshape(self.rows, self.n).to(DEV)
            assert w.dtype == t.dtype, (w.dtype, t.dtype)
            got = t[:, :self.n]
            assert torch.equal(got, w), E.report_mismatch(got, w, what)
            z = self.n
            if zero_pad:
                z = min(E.r8(self.n), self.ld)
                pad, zero = t[:, self.n:z], torch.zeros_like(t[:, self.n:z])
                assert torch.equal(pad, zero), E.report_mismatch(pad, zero, what + ": pad columns N..r8(N) not zero")
        self.check_guards(what, (("columns past the output", t[:, z:]),))

    def check_guards(self, what, more=()):
        """The guard bands still hold the sentinel (all that is asserted of a scratch buffer)."""
        for name, g in more + (("front guard", self.flat[None, :GUARD]), ("back guard", self.flat[None, -GUARD:])):
            s = torch.full_like(g, self.sent)
            assert torch.equal(g, s), E.report_mismatch(g, s, f"{what}: {name} written")


def _dev16(t, ld=None, fill=0.0):
    """CPU fp32 [rows, n] -> device bf16 [rows, ld], pad columns = fill."""
    assert E.bf16_exact(t)
    return E.pad_cols(t, ld or t.shape[1], fill).to(torch.bfloat16).to(DEV)


def _dev32(t, ld=None, fill=PAD_IN):
    t2 = t.reshape(1, -1) if t.dim() == 1 else t
    return E.pad_cols(t2.float(), ld or t2.shape[1], fill).to(DEV)


# ------------------------------------------------------------------------------------------ mmt_op_gemm
VARIANTS = [("default", -1, None)] + \
    [(hex(v), v, None) for v in (0x100 | 0x10000, 0x200 | 0x10000, 0x300 | 0x10000, 0x10000, 5, 2, 4, 0x20000 | 0x10000)] + \
    [("t2", 0x10000, 1)]
VARIANT_IDS = [v[0] for v in VARIANTS]
# shapes that also run with leading dimensions off the 16-byte grid (!vec_ok: the scalar epilogue on every column)
UNALIGNED = {(33, 17, 45), (200, 136, 72), (300, 264, 520)}
FWD_EPIS = ["store_f32", "bias_resid_f32", "store_bf16", "bias_relu_bf16"]
BWD_EPIS = ["store_f32", "acc_f32", "store_bf16", "drelu_bf16", "dtanh_bf16"]


@contextlib.contextmanager
def _variant(variant, t2):
    L = ML.lib()
    assert L.mmt_gemm_set_variant(variant) == 0
    old = L.mmt_gemm_set_t2(t2) if t2 is not None else None
    try:
        yield L
    finally:
        if t2 is not None:
            L.mmt_gemm_set_t2(old)
        L.mmt_gemm_set_variant(-1)


def _lds(N, aligned):
    """Leading dimensions of the epilogue operands: on the 16-byte grid with pad columns (the vector epilogue), or
    off it (bf16 not a multiple of 8, fp32 not a multiple of 4)."""
    if aligned:
        return dict(ldo16=E.r8(N) + 8, ldc=E.r4(N) + 4, ldaux=E.r8(N), ldres=E.r4(N))
    o16 = N + 1 if (N + 1) % 8 else N + 3
    o32 = N + 1 if (N + 1) % 4 else N + 2
    return dict(ldo16=o16, ldc=o32, ldaux=o16, ldres=o32)


def _layouts(M, N, K):
    return (True, False) if (M, N, K) in UNALIGNED else (True,)


@functools.lru_cache(maxsize=None)
def _fwd_dev(M, N, K, aligned):
    c, ld = E.gemm_fwd_case(M, N, K), _lds(N, aligned)
    return dict(X=_dev16(c["X"], E.r8(K)), W=_dev16(c["W"], E.r8(K)), bias=c["bias"].to(DEV),
                resid=_dev32(c["resid"], ld["ldres"]))


@functools.lru_cache(maxsize=None)
def _bwd_dev(M, N, K, aligned):
    c, ld = E.gemm_bwd_case(M, N, K), _lds(N, aligned)
    return dict(dY=_dev16(c["dY"], E.r8(K)), W=_dev16(c["W"], E.r8(N), PAD_IN),
                drelu_bf16=_dev16(c["aux_relu"], ld["ldaux"], PAD_IN), dtanh_bf16=_dev16(c["aux_tanh"], ld["ldaux"], PAD_IN))


@functools.lru_cache(maxsize=None)
def _wgrad_dev(M, N, R):
    c = E.gemm_wgrad_case(M, N, R)
    return dict(dY=_dev16(c["dY"], E.r8(M), PAD_IN), X=_dev16(c["X"], E.r8(N), PAD_IN))


@pytest.mark.parametrize("M,N,K", E.GEMM_SHAPES)
@pytest.mark.parametrize("name,variant,t2", VARIANTS, ids=VARIANT_IDS)
def test_gemm_forward_exact(name, variant, t2, M, N, K):
    """out = X W^T (+ bias, + residual, ReLU) under every pipeline variant: the vector and the scalar edge
    epilogue, ragged M, ragged K with K % 8 != 0, 1 to many K-tiles of BK 32 and 64."""
    c = E.gemm_fwd_case(M, N, K)
    with _variant(variant, t2) as L:
        for aligned in _layouts(M, N, K):
            d, ld = _fwd_dev(M, N, K, aligned), _lds(N, aligned)
            for epi in FWD_EPIS:
                o32 = _Buf(M, N, ld["ldc"], torch.float32)
                o16 = _Buf(M, N, ld["ldo16"], torch.bfloat16)
                rc = L.mmt_op_gemm(_s(), 1, 1, ML.EPI[epi], 1, M, N, K, ML.ptr(d["X"]), E.r8(K), ML.ptr(d["W"]), E.r8(K),
                                   ML.ptr(d["bias"]) if epi != "store_bf16" else None, None, 0, ML.ptr(d["resid"]),
                                   ld["ldres"], o32.ptr(), ld["ldc"], o16.ptr(), ld["ldo16"], 1.0)
                assert rc == 0
                w32, w16 = E.gemm_fwd_want(c, epi)
                what = f"forward {epi} {M}x{N}x{K} variant {name} aligned {aligned}"
                o32.check(w32, what + " o32")
                o16.check(w16, what + " o16", zero_pad=True)


@pytest.mark.parametrize("M,N,K", E.GEMM_SHAPES)
@pytest.mark.parametrize("name,variant,t2", VARIANTS, ids=VARIANT_IDS)
def test_gemm_backward_data_exact(name, variant, t2, M, N, K):
    """dX = alpha dY W (b_kc = 0; W's pad columns hold 1000), alpha 1 and 0.5: store, accumulate into an integer
    prefill (with its bf16 copy), ReLU' (aux > 0; +0 and -0 are not) and tanh' (1 - aux^2 in {1, 0.75, 0})."""
    c = E.gemm_bwd_case(M, N, K)
    with _variant(variant, t2) as L:
        for aligned in _layouts(M, N, K):
            d, ld = _bwd_dev(M, N, K, aligned), _lds(N, aligned)
            for epi in BWD_EPIS:
                for alpha in E.BWD_ALPHAS:
                    o32 = _Buf(M, N, ld["ldc"], torch.float32, c["prefill"] if epi == "acc_f32" else None)
                    o16 = _Buf(M, N, ld["ldo16"], torch.bfloat16)
                    aux = d.get(epi)
                    rc = L.mmt_op_gemm(_s(), 1, 0, ML.EPI[epi], 1, M, N, K, ML.ptr(d["dY"]), E.r8(K), ML.ptr(d["W"]),
                                       E.r8(N), None, ML.ptr(aux), ld["ldaux"], None, 0, o32.ptr(), ld["ldc"], o16.ptr(),
                                       ld["ldo16"], alpha)
                    assert rc == 0
                    w32, w16 = E.gemm_bwd_want(c, epi, alpha)
                    what = f"backward-data {epi} alpha {alpha} {M}x{N}x{K} variant {name} aligned {aligned}"
                    o32.check(w32, what + " o32")
                    o16.check(w16, what + " o16", zero_pad=True)


@pytest.mark.parametrize("M,N,K", E.GEMM_SHAPES)
@pytest.mark.parametrize("name,variant,t2", VARIANTS, ids=VARIANT_IDS)
def test_gemm_atomic_exact(name, variant, t2, M, N, K):
    """out += 0.25 dY[K, M]^T X[K, N] by float atomics (a_kc = 0, b_kc = 0; both operands' pad columns hold 1000)
    with 1, 4 and automatic K splits into an integer prefill: the same bits whatever the arrival order."""
    c, d = E.gemm_wgrad_case(M, N, K), _wgrad_dev(M, N, K)
    with _variant(variant, t2) as L:
        for aligned in _layouts(M, N, K):
            ldc = _lds(N, aligned)["ldc"]
            for splits in (1, 4, 0):
                o32 = _Buf(M, N, ldc, torch.float32, c["prefill"])
                rc = L.mmt_op_gemm(_s(), 0, 0, ML.EPI["atomic_f32"], splits, M, N, K, ML.ptr(d["dY"]), E.r8(M),
                                   ML.ptr(d["X"]), E.r8(N), None, None, 0, None, 0, o32.ptr(), ldc, None, 0, E.ATOMIC_ALPHA)
                assert rc == 0
                o32.check(c["want"], f"atomic_f32 splits {splits} {M}x{N}x{K} variant {name} aligned {aligned}")


@pytest.mark.parametrize("slabs", ["none", "auto", "three"])
@pytest.mark.parametrize("variant", [-1, 0x30000, 0x300])
@pytest.mark.parametrize("M,N,R", E.WGRAD_SHAPES)
def test_gemm_wgrad_exact(M, N, R, variant, slabs):
    """mmt_op_gemm_wgrad into an integer prefill. The split rule (mmt_launch_gemm_wgrad, auto_splits): about 128
    blocks per launch, at most 32 splits, at least 512 K rows per split, never more than the slab holds; without a
    slab, or with one split, one K pass accumulates straight into out. So (450, 256, 3000) gets 5 slabs with a
    roomy slab ("auto") and 3 with a slab of three ("three"), (384, 256, 4096) 8 and 3, each followed by the reduce
    pass; (6, 32, 300) and (33, 45, 77) (K < 1024: one split) and every shape without a slab ("none") take one pass.
    Variants: the default ring, the ping-pong 256 x 256 kernel (0x30000), the 256 x 256 ring at BK 32 x 2 (0x300).
    Both a 16-byte-aligned and an odd leading dimension of out (the reduce pass's scalar form)."""
    c, d = E.gemm_wgrad_case(M, N, R), _wgrad_dev(M, N, R)
    per = (M * N + 3) // 4 * 4
    nfl = {"none": 0, "auto": 32 * per, "three": 3 * per}[slabs]
    with _variant(variant, None) as L:
        for ldc in (E.r4(N) + 4, N + 1 if (N + 1) % 4 else N + 2):
            out = _Buf(M, N, ldc, torch.float32, c["prefill"])
            slab = _Buf(1, nfl, nfl, torch.float32) if nfl else None
            rc = L.mmt_op_gemm_wgrad(_s(), M, N, R, ML.ptr(d["dY"]), E.r8(M), ML.ptr(d["X"]), E.r8(N), out.ptr(), ldc,
                                     E.ATOMIC_ALPHA, slab.ptr() if slab else None, 4 * nfl)
            assert rc == 0
            what = f"wgrad {M}x{N}x{R} variant {variant:#x} slabs {slabs} ldc {ldc}"
            out.check(c["want"], what)
            if slab:  # scratch: its contents are unspecified, its surroundings are not
                slab.check_guards(what + " slab")


# ------------------------------------------------------------------------------- column sums, ordered sum
@pytest.mark.parametrize("R,N,ld", [(1000, 450, 456), (77, 13, 16), (300, 6, 8), (520, 264, 272), (300, 45, 47)])
def test_colsum_exact(R, N, ld):
    """out[n] += 0.5 sum_r x[r, n] by one atomic per 256-row block, ld > N (pad columns 1000), prefilled out."""
    c = E.colsum_case(R, N, ld)
    x = _dev16(c["x"], ld, PAD_IN)
    out = _Buf(1, N, N + 8, torch.float32, c["prefill"])
    assert ML.lib().mmt_op_colsum(_s(), R, N, ML.ptr(x), ld, out.ptr(), 0.5) == 0
    out.check(c["want"], f"colsum {R}x{N} ld {ld}")


@pytest.mark.parametrize("nparts,n", [(1, 13), (5, 300), (40, 300), (33, 1)])
def test_ordered_sum_exact(nparts, n):
    """dst[i] += the partials in index order (one, fewer and more than the 32 loaded ahead), ld > n, prefilled."""
    c = E.ordered_sum_case(nparts, n)
    ld = n + 5
    parts = _dev32(c["parts"], ld)
    dst = _Buf(1, n, n + 8, torch.float32, c["prefill"])
    assert ML.lib().mmt_op_ordered_sum(_s(), nparts, n, ML.ptr(parts), ld, dst.ptr()) == 0
    dst.check(c["want"], f"ordered_sum {nparts}x{n}")


# ------------------------------------------------------------------------------------ per-head stage 2
@pytest.mark.parametrize("coal", [3, 0])
@pytest.mark.parametrize("R,H,hs", E.QKV2_SHAPES)
def test_qkv2_exact(R, H, hs, coal):
    """mmt_op_qkv2_fwd / _bwd at hs 8, 16, 32, 64: forward rows, dh1 = RNE((dout bf16(W2)) (1 - h1^2)) and dW2
    into an integer prefill. dW2 is added by atomics, one per element per 1024-row block at hs 32 / 64 ((1055, 3, 32)
    and (1100, 2, 64): two blocks, the second ragged; (33, 2, 64) ends one row into a 32-row tile): exact all the
    same. Pad columns of h1 / dout hold 1000; those of out / dh1 are not written."""
    c = E.qkv2_case(R, H, hs)
    nblk, hh = 3 * H, hs // 2
    ld_h1, ld_out = E.r8(nblk * hh) + 8, nblk * hs + 8
    h1 = _dev16(c["h1"].reshape(R, nblk * hh), ld_h1, PAD_IN)
    dout = _dev16(c["dout"].reshape(R, nblk * hs), ld_out, PAD_IN)
    w2 = c["w2"].to(DEV)
    L = ML.lib()
    old = L.mmt_qkv2_set_coal(coal)
    try:
        out = _Buf(R, nblk * hs, ld_out, torch.bfloat16)
        assert L.mmt_op_qkv2_fwd(_s(), R, nblk, hs, ML.ptr(h1), ld_h1, ML.ptr(w2), out.ptr(), ld_out) == 0
        out.check(c["out"], f"qkv2 forward R {R} H {H} hs {hs}")
        dh1 = _Buf(R, nblk * hh, ld_h1, torch.bfloat16)
        dw2 = _Buf(1, nblk * hs * hh, nblk * hs * hh, torch.float32, c["pre"])
        assert L.mmt_op_qkv2_bwd(_s(), R, nblk, hs, ML.ptr(h1), ld_h1, ML.ptr(w2), ML.ptr(dout), ld_out, dh1.ptr(),
                                 dw2.ptr()) == 0
        dh1.check(c["dh1"], f"qkv2 dh1 R {R} H {H} hs {hs} coal {coal}")
        dw2.check(c["dw2"], f"qkv2 dW2 R {R} H {H} hs {hs} coal {coal}")
    finally:
        L.mmt_qkv2_set_coal(old)


# -------------------------------------------------------------------------------- out-projection backward
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("M,C", E.MLP2_BWD_CASES)
def test_mlp2_bwd_exact(M, C, alpha):
    """mmt_op_mlp2_bwd: dh = RNE(d), d = alpha (dy W2) (1 - h^2); dx = RNE(dh16 W0) from the stored bf16 dh;
    db0 += the column sums of d in fp32 BEFORE the bf16 store (the kernel adds up its fp32 registers, not the
    stored values; on these inputs the two conventions differ in most columns and the other one fails).
    Every operand has pad columns (1000); dh has pad columns that stay untouched."""
    c = E.mlp2_bwd_case(M, C, alpha)
    N1 = C // 2
    assert int((c["db0"].double() != c["db0_stored"]).sum()) > N1 // 4  # the inputs tell the conventions apart
    dy, w2 = _dev16(c["dy"], C + 8, PAD_IN), _dev16(c["w2"], N1 + 8, PAD_IN)
    h, w0 = _dev16(c["h"], N1 + 4, PAD_IN), _dev16(c["w0"], C + 8, PAD_IN)
    dh = _Buf(M, N1, N1 + 8, torch.bfloat16)
    dx = _Buf(M, C, C, torch.bfloat16)
    db0 = _Buf(1, N1, N1 + 8, torch.float32, c["pre"])
    rc = ML.lib().mmt_op_mlp2_bwd(_s(), M, C, ML.ptr(dy), C + 8, ML.ptr(w2), N1 + 8, ML.ptr(h), N1 + 4, alpha, ML.ptr(w0),
                                  C + 8, dh.ptr(), N1 + 8, db0.ptr(), dx.ptr())
    assert rc == 0
    what = f"mlp2_bwd M {M} C {C} alpha {alpha}"
    dh.check(c["dh"], what + " dh")
    db0.check(c["db0"], what + " db0 (fp32 sums before the bf16 store)")
    dx.check(c["dx"], what + " dx")


# ------------------------------------------------------------------------------------------ FFN forward
@functools.lru_cache(maxsize=None)
def _ffn_dev():
    w = E.ffn_weights()
    g = torch.Generator().manual_seed(45)
    return dict(w0=_dev16(w["w0"], E.FFN_C + 8, PAD_IN), b0=w["b0"].to(DEV), w2=_dev16(w["w2"], E.FFN_HID + 8, PAD_IN),
                b2=w["b2"].to(DEV), g=torch.randn(E.FFN_C, generator=g).to(DEV), be=torch.randn(E.FFN_C, generator=g).to(DEV))


@pytest.mark.parametrize("lnf", [False, True])
@pytest.mark.parametrize("Ms", [(37,), (37, 128, 200)])
def test_ffn_exact(Ms, lnf):
    """mmt_op_ffn at C = 256, one and three problems with ragged row counts, dropout off: h = RNE(relu(x W0^T + b0))
    (b0 lifts values past 256: rounded), out = resid + h16 W2^T + b2 exact in fp32, out16 = RNE(out). With the fused
    LayerNorm only h, out and out16 are asserted (its outputs go through rsqrt). The unfused pair
    mmt_op_gemm(bias_relu_bf16) + mmt_op_gemm(bias_resid_f32) gives the same bits on the same inputs."""
    C, HID = E.FFN_C, E.FFN_HID
    ldx, ldh, ldw0, ldw2 = C + 16, HID + 24, C + 8, HID + 8
    w, L, n = _ffn_dev(), ML.lib(), len(Ms)
    cs = [E.ffn_case(M, 100 * i + M) for i, M in enumerate(Ms)]
    x = [_dev16(c["x"], ldx, PAD_IN) for c in cs]
    resid = [c["resid"].to(DEV) for c in cs]
    h = [_Buf(M, HID, ldh, torch.bfloat16) for M in Ms]
    out = [_Buf(M, C, C, torch.float32) for M in Ms]
    out16 = [_Buf(M, C, C, torch.bfloat16) for M in Ms]
    ly = [torch.zeros(M, C, dtype=torch.bfloat16, device=DEV) for M in Ms]
    lm, lr = [torch.zeros(M, device=DEV) for M in Ms], [torch.zeros(M, device=DEV) for M in Ms]
    arr = lambda ts: ML.ptr_array([t.t if isinstance(t, _Buf) else t for t in ts])
    rc = L.mmt_op_ffn(_s(), n, (ctypes.c_int32 * n)(*Ms), C, arr(x), ldx, ML.ptr(w["w0"]), ldw0, ML.ptr(w["b0"]),
                      ML.ptr(w["w2"]), ldw2, ML.ptr(w["b2"]), arr(h), ldh, arr(resid), arr(out), arr(out16), 0, 0, 1.0,
                      ML.ptr(w["g"]) if lnf else None, ML.ptr(w["be"]) if lnf else None, arr(ly) if lnf else None,
                      arr(lm) if lnf else None, arr(lr) if lnf else None)
    assert rc == 0
    for i, (M, c) in enumerate(zip(Ms, cs)):
        what = f"ffn problem {i} of {Ms} M {M} lnf {lnf}"
        h[i].check(c["h"], what + " h")
        out[i].check(c["out"], what + " out")
        out16[i].check(c["out16"], what + " out16")
        # the pair of launches it replaces
        h2, o2, o16 = _Buf(M, HID, ldh, torch.bfloat16), _Buf(M, C, C, torch.float32), _Buf(M, C, C, torch.bfloat16)
        assert L.mmt_op_gemm(_s(), 1, 1, ML.EPI["bias_relu_bf16"], 1, M, HID, C, ML.ptr(x[i]), ldx, ML.ptr(w["w0"]), ldw0,
                             ML.ptr(w["b0"]), None, 0, None, 0, None, 0, h2.ptr(), ldh, 1.0) == 0
        assert L.mmt_op_gemm(_s(), 1, 1, ML.EPI["bias_resid_f32"], 1, M, C, HID, h2.ptr(), ldh, ML.ptr(w["w2"]), ldw2,
                             ML.ptr(w["b2"]), None, 0, ML.ptr(resid[i]), C, o2.ptr(), C, o16.ptr(), C, 1.0) == 0
        h2.check(c["h"], what + " pair h")
        o2.check(c["out"], what + " pair out")
        o16.check(c["out16"], what + " pair out16")


# --------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("B,T,C,V", E.EMB_SHAPES)
def test_embedding_exact(B, T, C, V):
    """x = tok[idx] + pos; dtok += the rows of dx by token, dpos += their sums over the batch, both into integer
    prefills (float atomics in any order: exact on integers)."""
    c, L = E.embedding_case(B, T, C, V), ML.lib()
    idx, tok, pos, dx = c["idx"].to(DEV), c["tok"].to(DEV), c["pos"].to(DEV), c["dx"].to(DEV)
    x = _Buf(B * T, C, C, torch.float32)
    assert L.mmt_op_embedding_fwd(_s(), B, T, C, V, ML.ptr(idx), ML.ptr(tok), ML.ptr(pos), x.ptr()) == 0
    x.check(c["x"], f"embedding forward {B, T, C, V}")
    dtok, dpos = _Buf(V, C, C, torch.float32, c["dtok0"]), _Buf(T, C, C, torch.float32, c["dpos0"])
    assert L.mmt_op_embedding_bwd(_s(), B, T, C, V, ML.ptr(idx), ML.ptr(dx), dtok.ptr(), dpos.ptr()) == 0
    dtok.check(c["dtok"], f"embedding dtok {B, T, C, V}")
    dpos.check(c["dpos"], f"embedding dpos {B, T, C, V}")


@pytest.mark.parametrize("sort", [1, 0])
@pytest.mark.parametrize("B,T,C,V", E.EMB_SHAPES)
def test_embedding_bwd_ws_exact(B, T, C, V, sort):
    """The scratch path (the engine's): counting sort + run sums (sort 1) and the LDS-privatised slabs with
    per-chunk partial tables, the atomic flush and direct atomics (sort 0), torch.equal where the random-input
    tests allow 1e-4 / 1e-3. The scratch's surroundings stay untouched."""
    c, L = E.embedding_case(B, T, C, V), ML.lib()
    idx, dx = c["idx"].to(DEV), c["dx"].to(DEV)
    dtok, dpos = _Buf(V, C, C, torch.float32, c["dtok0"]), _Buf(T, C, C, torch.float32, c["dpos0"])
    scratch = _Buf(1, B * T * C, B * T * C, torch.float32)
    old = L.mmt_emb_set_sort(sort)
    try:
        assert L.mmt_op_embedding_bwd_ws(_s(), B, T, C, V, ML.ptr(idx), ML.ptr(dx), dtok.ptr(), dpos.ptr(),
                                         scratch.ptr()) == 0
    finally:
        L.mmt_emb_set_sort(old)
    dtok.check(c["dtok"], f"embedding_bwd_ws dtok {B, T, C, V} sort {sort}")
    dpos.check(c["dpos"], f"embedding_bwd_ws dpos {B, T, C, V} sort {sort}")
    scratch.check_guards(f"embedding_bwd_ws scratch {B, T, C, V} sort {sort}")


# ------------------------------------------------------------------------------------------- MX-fp8 GEMM
@pytest.mark.parametrize("M,N,K", E.F8_SHAPES)
def test_gemm_f8_exact(M, N, K):
    """mmt_op_gemm_f8 on e4m3 bytes of small integers with hand-set E8M0 bytes (0.5, 1, 2) that differ per row and
    per 32-column block: an exponent applied to the wrong block or row changes the answer. store_f32 with bias is
    exact; bias_relu_bf16 gives o16 = RNE(relu) and, where N % 32 == 0 (the entry refuses o8 otherwise), o8 / s8
    equal to the oracle's mx_fp8_parts of the exact fp32 value, byte for byte."""
    import mmt_oracle as O
    c, L = E.f8_case(M, N, K), ML.lib()
    lda = K + 16
    a8 = E.pad_cols(c["a8"], lda, 0x38).to(DEV)
    b8 = E.pad_cols(c["b8"], lda, 0x38).to(DEV)
    sa, sb, bias = c["sa"].to(DEV), c["sb"].to(DEV), c["bias"].to(DEV)
    ldc, ldo16 = E.r4(N) + 4, E.r8(N) + 8
    o32 = _Buf(M, N, ldc, torch.float32)
    assert L.mmt_op_gemm_f8(_s(), ML.EPI["store_f32"], M, N, K, ML.ptr(a8), lda, ML.ptr(sa), c["lds"], ML.ptr(b8), lda,
                            ML.ptr(sb), c["lds"], ML.ptr(bias), None, 0, o32.ptr(), ldc, None, 0, None, 0, None, 0) == 0
    o32.check(c["v"], f"gemm_f8 store_f32 {M}x{N}x{K}")
    mx = N % 32 == 0
    o16 = _Buf(M, N, ldo16, torch.bfloat16)
    o8 = _Buf(M, N, N + 8, torch.uint8) if mx else None
    s8 = _Buf(M, N // 32, N // 32 + 4, torch.uint8) if mx else None
    assert L.mmt_op_gemm_f8(_s(), ML.EPI["bias_relu_bf16"], M, N, K, ML.ptr(a8), lda, ML.ptr(sa), c["lds"], ML.ptr(b8),
                            lda, ML.ptr(sb), c["lds"], ML.ptr(bias), None, 0, None, 0, o16.ptr(), ldo16,
                            o8.ptr() if mx else None, N + 8, s8.ptr() if mx else None, N // 32 + 4) == 0
    o16.check(E.rne_bf16(c["relu"]), f"gemm_f8 bias_relu_bf16 {M}x{N}x{K} o16", zero_pad=True)
    if mx:
        q, e = O.mx_fp8_parts(c["relu"])
        o8.check(q.view(torch.uint8), f"gemm_f8 bias_relu_bf16 {M}x{N}x{K} o8")
        s8.check((e + 127).to(torch.uint8), f"gemm_f8 bias_relu_bf16 {M}x{N}x{K} s8")
