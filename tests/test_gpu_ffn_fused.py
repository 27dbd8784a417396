"""The FFN forward as one launch at C = 256 (mmt_op_ffn / mmt_set_ffn_fused, include/mmt.h; ffn_fwd_kernel:
Linear(C, 4C) -> ReLU -> Linear(4C, C) -> hash dropout -> + residual -> optional next LayerNorm, the hidden
activation walked through LDS in 128-column chunks; reference model.py:162-175, 225).

Three views of it:
  * against torch on the same bf16 operands, with the project's bounds (h as test_gemm_forward_linear's bias_relu
    bound, the rest as test_mlp2_fused): ragged and multi-tile row counts, dropout, LayerNorm, the bf16 copy, padded
    leading dimensions, a grouped launch with an empty-tile problem, and a full-chip launch (512 workgroups, two
    generations: where a miscounted vmcnt wait shows);
  * bitwise against the pair of launches it replaces (mmt_op_gemm bias_relu_bf16, then bias_resid_f32): stage 1
    uses ffn0's MFMA and K order, stage 2 the ping-pong kernel's 16x16x32 K slots in one ascending accumulator, so
    h, the fp32 output and the bf16 copy carry the same bits;
  * in the engine: knob 0 against knob 1 on the C = 256 golden (forward bitwise, gradient within the run-to-run
    bound, bitwise in deterministic mode), no launch at other widths or with ReLU bits on.
"""
import ctypes
import functools

import pytest
import torch

import config_utils
import mmt_lib as ML
from golden_io import model_fixture, scale_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 256
HID = 4 * C
KEY = 0x2468ACE
GRAD_BOUND = 1e-6  # tests/test_gpu_determinism.py: the same sums in another order
UNSUPPORTED = -2


def _s():
    return ML.stream_ptr()


def rel(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def bf(t):
    return t.to(torch.bfloat16).contiguous()


@functools.lru_cache(maxsize=None)
def _weights():
    """The shared operands: weights, biases, LayerNorm parameters (made once, never modified)."""
    g = torch.Generator(device=DEV).manual_seed(8)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    return dict(w0=bf(rn(HID, C) * 0.05), b0=rn(HID) * 0.1, w2=bf(rn(C, HID) * 0.05), b2=rn(C) * 0.1, g=rn(C), be=rn(C))


@functools.lru_cache(maxsize=None)
def _keep(M, drop):
    """The hash-dropout keep-and-scale factor [M][C] of KEY (host hash, made once per shape), and the oracle's
    threshold and scale."""
    import mmt_oracle as O
    hd = O.HashDropout(11, drop)
    rows = torch.arange(M).numpy()[:, None]
    cols = torch.arange(C).numpy()[None, :]
    return hd._mask(KEY, rows, cols).to(DEV), hd.thr, hd.scale


def _inputs(Ms, seed, ldx=C, ldh=HID):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for M in Ms:
        xf = torch.zeros(M, ldx, device=DEV)
        xf[:, :C] = torch.randn(M, C, device=DEV, generator=g)
        if ldx > C:
            xf[:, C:] = 7.0  # pad columns must not be read
        out.append(dict(M=M, x=bf(xf), resid=torch.randn(M, C, device=DEV, generator=g),
                        h=torch.full((M, ldh), -3.0, dtype=torch.bfloat16, device=DEV),
                        out=torch.zeros(M, C, device=DEV), out16=torch.zeros(M, C, dtype=torch.bfloat16, device=DEV),
                        ly=torch.zeros(M, C, dtype=torch.bfloat16, device=DEV), lm=torch.zeros(M, device=DEV),
                        lr=torch.zeros(M, device=DEV)))
    return out


def _ffn(ps, drop, lnf, copy, ldx=C, ldh=HID, c=C, x_ptrs=None):
    w = _weights()
    n = len(ps)
    thr, scale = (_keep(1, drop)[1:] if drop else (0, 1.0))
    Ms = (ctypes.c_int32 * n)(*[p["M"] for p in ps])
    arr = lambda k: ML.ptr_array([p[k] for p in ps])
    xs = arr("x")
    if x_ptrs is not None:
        for i, v in enumerate(x_ptrs):
            xs[i] = v
    return ML.lib().mmt_op_ffn(_s(), n, Ms, c, xs, ldx, ML.ptr(w["w0"]), C, ML.ptr(w["b0"]), ML.ptr(w["w2"]), HID,
                               ML.ptr(w["b2"]), arr("h"), ldh, arr("resid"), arr("out"), arr("out16") if copy else None,
                               KEY, thr, scale, ML.ptr(w["g"]) if lnf else None, ML.ptr(w["be"]) if lnf else None,
                               arr("ly") if lnf else None, arr("lm") if lnf else None, arr("lr") if lnf else None)


def _check(p, drop, lnf, copy, ldh=HID):
    w = _weights()
    M = p["M"]
    x = p["x"][:, :C].float()
    href = torch.relu(x @ w["w0"].float().t() + w["b0"])
    h = p["h"][:, :HID]
    e_h = rel(h, href)
    y = h.float() @ w["w2"].float().t() + w["b2"]  # the kernel's own bf16 h as the second operand
    if drop:
        y = y * _keep(M, drop)[0]
    ref = p["resid"] + y
    e_o = rel(p["out"], ref)
    print(f"M {M} drop {drop} lnf {lnf} copy {copy}: h rel {e_h:.3e} out rel {e_o:.3e}")
    assert e_h < 1e-2
    assert e_o < 1e-4
    if ldh > HID:
        assert bool((p["h"][:, HID:] == -3.0).all())  # pad columns of h untouched
    if copy:
        assert rel(p["out16"], ref) < 1e-2
    else:
        assert not bool(p["out16"].any())
    if lnf:
        lref = torch.nn.functional.layer_norm(p["out"], (C,), w["g"], w["be"], 1e-5)
        assert rel(p["ly"], lref) < 1e-2
        assert rel(p["lm"], p["out"].mean(1)) < 1e-5
    else:
        assert not bool(p["ly"].any())


@pytest.mark.parametrize("M,drop,lnf,copy,pad", [
    (97, 0.0, False, False, False), (97, 0.1, True, True, False), (300, 0.1, True, False, False),
    (300, 0.0, False, True, True), (1000, 0.1, False, True, False), (1000, 0.0, True, False, False)])
def test_ffn_fused_against_torch(M, drop, lnf, copy, pad):
    """One problem: one ragged tile (97), three tiles with a ragged last (300), 1000 rows; dropout, LayerNorm and
    the bf16 copy on and off; pad: ldx > C and ldh > 4C (pad columns neither read nor written)."""
    ldx, ldh = (C + 16, HID + 24) if pad else (C, HID)
    ps = _inputs([M], M, ldx, ldh)
    assert _ffn(ps, drop, lnf, copy, ldx, ldh) == 0
    torch.cuda.synchronize()
    _check(ps[0], drop, lnf, copy, ldh)


def test_ffn_fused_grouped_launch():
    """Four problems in one launch, M = (97, 128, 300, 1): blockIdx.z, and workgroups past a problem's last
    tile leave at once."""
    ps = _inputs([97, 128, 300, 1], 5)
    assert _ffn(ps, 0.1, True, True) == 0
    torch.cuda.synchronize()
    for p in ps:
        _check(p, 0.1, True, True)


@functools.lru_cache(maxsize=None)
def _full_chip():
    """The C1 grouping, 4 problems x 16384 rows (512 workgroups), dropout and LayerNorm on: run once, shared."""
    ps = _inputs([16384] * 4, 6)
    assert _ffn(ps, 0.1, True, True) == 0
    torch.cuda.synchronize()
    return ps


def test_ffn_fused_full_chip_against_torch():
    for p in _full_chip():
        _check(p, 0.1, True, True)
        assert bool(torch.isfinite(p["out"]).all())


def _pair(p):
    """The two launches the fused one replaces, on p's inputs: (h, out, out16)."""
    w = _weights()
    M = p["M"]
    L = ML.lib()
    h = torch.zeros(M, HID, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(M, C, device=DEV)
    out16 = torch.zeros(M, C, dtype=torch.bfloat16, device=DEV)
    assert L.mmt_op_gemm(_s(), 1, 1, ML.EPI["bias_relu_bf16"], 1, M, HID, C, ML.ptr(p["x"]), C, ML.ptr(w["w0"]), C,
                         ML.ptr(w["b0"]), None, 0, None, 0, None, 0, ML.ptr(h), HID, 1.0) == 0
    assert L.mmt_op_gemm(_s(), 1, 1, ML.EPI["bias_resid_f32"], 1, M, C, HID, ML.ptr(h), HID, ML.ptr(w["w2"]), HID,
                         ML.ptr(w["b2"]), None, 0, ML.ptr(p["resid"]), C, ML.ptr(out), C, ML.ptr(out16), C, 1.0) == 0
    torch.cuda.synchronize()
    return h, out, out16


def _assert_pair_bits(p):
    h, out, out16 = _pair(p)
    dh = int((h != p["h"]).sum().item())
    do = int((out != p["out"]).sum().item())
    print(f"M {p['M']}: h entries differing {dh}, out entries differing {do}")
    assert torch.equal(h, p["h"])
    assert torch.equal(out, p["out"])
    assert torch.equal(out16, p["out16"])


def test_ffn_fused_bitwise_against_pair():
    """M = 300 (ffn2 on the ping-pong kernel: M, N >= 256 and K = 1024), no dropout (mmt_op_gemm has none)."""
    ps = _inputs([300], 300)
    assert _ffn(ps, 0.0, False, True) == 0
    torch.cuda.synchronize()
    _assert_pair_bits(ps[0])


def test_ffn_fused_full_chip_bitwise_against_pair():
    """The full-chip grouping without dropout against the pair, problem by problem (same inputs as _full_chip)."""
    ps = _inputs([16384] * 4, 6)
    assert _ffn(ps, 0.0, False, True) == 0
    torch.cuda.synchronize()
    for p in ps:
        _assert_pair_bits(p)
    # and the dropout / LayerNorm run of the same inputs made the same h
    for p, q in zip(ps, _full_chip()):
        assert torch.equal(p["h"], q["h"])


def test_ffn_op_refusals_launch_nothing():
    """C = 512 and a pointer off 16-B alignment return MMT_ERR_UNSUPPORTED, and no output is touched."""
    ps = _inputs([300], 9)
    assert _ffn(ps, 0.0, False, True, c=512) == UNSUPPORTED
    assert _ffn(ps, 0.0, False, True, x_ptrs=[ps[0]["x"].data_ptr() + 2]) == UNSUPPORTED
    assert _ffn(ps, 0.0, False, True, ldx=C + 4) == UNSUPPORTED  # a leading dimension off 16 B
    torch.cuda.synchronize()
    p = ps[0]
    assert bool((p["h"] == -3.0).all()) and not bool(p["out"].any()) and not bool(p["out16"].any())


# ------------------------------------------------------------------------------------- engine
def _build(meta, sd, dropout, precision="bf16"):
    config_utils._config_cache = {"n_embd": meta["n_embd"], "n_head": meta["n_head"], "n_layer": meta["n_layer"],
                                  "block_size": meta["block_size"], "dropout": dropout, "device": "cuda",
                                  "batch_size": meta["B"], "eval_iters": 1, "precision": precision}
    import model as mmt_model
    m = mmt_model.MultimodalTransformer(len(meta["V"]), meta["V"], [[None] * 8 + [c] + [None] * 3 for c in meta["cross"]]).to("cuda")
    full = {k: t for k, t in m.state_dict().items() if k.endswith("tril")}
    full.update(sd)
    m.load_state_dict(full, strict=True)
    m._next_dropout_seed = lambda dev: 0x5EED1234  # the same masks on every forward
    m.train()
    return m


def _fwd_bwd(m, idx, tgt):
    m.flat_params.grad = None
    logits, losses = m(idx, tgt)
    sum(losses).backward()
    torch.cuda.synchronize()
    return ([l.detach().clone() for l in logits], torch.stack([l.detach() for l in losses]).clone(),
            m.flat_params.grad.detach().clone())


def _fixture(name):
    return scale_fixture(name) if name in ("f_c1", "f_m8", "f_t1024") else model_fixture(name)


def _with_knob(v, fn):
    L = ML.lib()
    old = L.mmt_set_ffn_fused(v)
    try:
        return fn()
    finally:
        L.mmt_set_ffn_fused(old)


def _probe_counts(m, idx, tgt, labels=("ffn", "ffn0", "ffn2")):
    """Launches per probe label over one forward + backward."""
    L = ML.lib()
    L.mmt_probe_set(m._ctx, ",".join(labels).encode())
    L.mmt_probe_enable(m._ctx, 1)
    try:
        _fwd_bwd(m, idx, tgt)
        out = {}
        for i, lab in enumerate(labels):
            ms, n, fl, by = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
            ML.check(L.mmt_probe_read_at(m._ctx, i, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by)),
                     m._ctx, "mmt_probe_read_at")
            out[lab] = n.value
        return out
    finally:
        L.mmt_probe_set(m._ctx, None)


@pytest.mark.parametrize("dropout", [0.1, 0.0])
def test_engine_knob_same_forward_bits(dropout):
    """f_c1 (the only golden with n_embd 256): the one-launch FFN against the ffn0 + ffn2 pair in the same
    context (the knob is read at every forward). Losses and logits bitwise; the gradient within the run-to-run
    bound of tests/test_gpu_determinism.py, and bitwise in deterministic mode. The path is taken (probe "ffn":
    one launch per layer) and the pair's labels then see none."""
    z, meta, cfg, sd, idx, tgt = _fixture("f_c1")
    assert meta["n_embd"] == C
    m = _build(meta, sd, dropout)
    idx_d, tgt_d = [t.cuda() for t in idx], [t.cuda() for t in tgt]
    for det in (False, True):
        m.set_deterministic(det)
        lg0, ls0, g0 = _with_knob(0, lambda: _fwd_bwd(m, idx_d, tgt_d))
        lg1, ls1, g1 = _with_knob(1, lambda: _fwd_bwd(m, idx_d, tgt_d))
        assert torch.equal(ls0, ls1), (ls0, ls1)
        for a, b in zip(lg0, lg1):
            assert torch.equal(a, b)
        err = ((g1 - g0).norm() / (g0.norm() + 1e-30)).item()
        print(f"f_c1 dropout {dropout} det {det}: grad rel-L2 knob 0 vs 1 {err:.3e}")
        if det:
            assert torch.equal(g0, g1)
        else:
            assert err <= GRAD_BOUND, err
    n1 = _with_knob(1, lambda: _probe_counts(m, idx_d, tgt_d))
    n0 = _with_knob(0, lambda: _probe_counts(m, idx_d, tgt_d))
    assert n1 == {"ffn": meta["n_layer"], "ffn0": 0, "ffn2": 0}, n1
    assert n0["ffn"] == 0 and n0["ffn0"] >= meta["n_layer"] and n0["ffn2"] >= meta["n_layer"], n0


def test_engine_eval_forward_takes_the_path():
    """Eval forwards (no dropout, no backward) run the one launch too, with the pair's bits."""
    z, meta, cfg, sd, idx, tgt = _fixture("f_c1")
    m = _build(meta, sd, 0.0)
    m.eval()
    idx_d, tgt_d = [t.cuda() for t in idx], [t.cuda() for t in tgt]

    def fwd():
        with torch.no_grad():
            logits, losses = m(idx_d, tgt_d)
        torch.cuda.synchronize()
        return [l.clone() for l in logits], torch.stack(list(losses)).clone()
    lg0, ls0 = _with_knob(0, fwd)
    lg1, ls1 = _with_knob(1, fwd)
    assert torch.equal(ls0, ls1)
    for a, b in zip(lg0, lg1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name,precision", [("f_small", "bf16"), ("f_hs32", "bf16"), ("f_m8", "bf16"), ("f_m8", "fp8")])
def test_engine_other_widths_keep_the_pair(name, precision):
    """Goldens of other widths (64, 128) and the fp8 path: the knob at 1 launches nothing under "ffn"."""
    z, meta, cfg, sd, idx, tgt = _fixture(name)
    assert meta["n_embd"] != C
    m = _build(meta, sd, 0.1, precision)
    n = _with_knob(1, lambda: _probe_counts(m, [t.cuda() for t in idx], [t.cuda() for t in tgt]))
    assert n["ffn"] == 0 and n["ffn0"] >= meta["n_layer"], n


def test_engine_relu_bits_keep_the_pair():
    """ReLU bits on (latched by mmt_create): ffn0 writes them in its epilogue, so the pair runs at C = 256 too."""
    z, meta, cfg, sd, idx, tgt = _fixture("f_c1")
    L = ML.lib()
    old = L.mmt_set_relu_bits(1)
    try:
        m = _build(meta, sd, 0.1)
    finally:
        L.mmt_set_relu_bits(old)
    n = _with_knob(1, lambda: _probe_counts(m, [t.cuda() for t in idx], [t.cuda() for t in tgt]))
    assert n["ffn"] == 0 and n["ffn0"] >= meta["n_layer"] and n["ffn2"] >= meta["n_layer"], n
