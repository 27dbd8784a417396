"""Sample fan-out on the GPU: generate(num_samples=S).

Kernel level: attn_decode_fanout_kernel<HS> through mmt_op_attention_decode_fanout against the fp64 reference of
tests/fanout_ref.py, every element under its derived bound, in the engine's two layouts. Every cache row at a
position >= n0, every tail row above pos - n0, every pad column and the whole tail, query and output row of a
guard sample after row B*S are NaN (the output's: a sentinel that must survive). tests/test_fanout_ref_cpu.py shows
that the planted bugs leave the bound on these inputs.

Engine level: mmt_decode_fanout_step under teacher forcing against the full forward and the CPU oracle with the
criteria of test_gpu_decode.py, the workspace left untouched, and generate(num_samples=S) end to end.
"""
import ctypes

import pytest
import torch

import config_utils
import fanout_ref as F
import mmt_lib as ML
from golden_io import model_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
SENTINEL = -77.0  # exact in bf16
O_PAD = 8
G = F.G
HEAD_SIZES = (8, 16, 24, 32, 48, 64)
LAYOUTS = ("self", "cross")


def rel(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# --------------------------------------------------------------------------------------- kernel level
def _pack(layout, q, ks, vs, tks, tvs, n0, t, T):
    """The canonical tensors in one of the engine's layouts, on the device, NaN wherever the kernel must not read:
    cache rows >= n0, tail rows > t - n0, pad columns, and one guard sample after row B*S."""
    B, S, H, hs = q.shape
    C, R, L = H * hs, B * S, t - n0 + 1
    cap = tks[0].shape[3]
    assert cap > L  # at least one poisoned tail row
    if layout == "self":
        q_ld = kv_ld = t_ld = 3 * C
        kv_hs, qo, ko, vo = hs, C, 0, 2 * C
    else:
        q_ld, kv_ld, t_ld = C + 8, 2 * C + 8, 2 * C + 8
        kv_hs, qo, ko, vo = 2 * hs, 0, 0, hs
    qbuf = torch.full((R + 1, q_ld), NAN, dtype=BF)
    qbuf[:R, qo:qo + C] = q.reshape(R, C)
    qbuf = qbuf.to(DEV)
    caches, tails = [], []
    for k, v, tk, tv in zip(ks, vs, tks, tvs):
        c = torch.full((B, T, kv_ld), NAN, dtype=BF)
        kk, vv = k[:, :, :n0].permute(0, 2, 1, 3), v[:, :, :n0].permute(0, 2, 1, 3)  # [B, n0, H, hs]
        tkk, tvv = tk[:, :, :, :L].permute(0, 1, 3, 2, 4), tv[:, :, :, :L].permute(0, 1, 3, 2, 4)  # [B, S, L, H, hs]
        tl = torch.full((R + 1, cap, t_ld), NAN, dtype=BF)
        if layout == "self":
            c[:, :n0, :C] = kk.reshape(B, n0, C)
            c[:, :n0, 2 * C:] = vv.reshape(B, n0, C)
            tl[:R, :L, :C] = tkk.reshape(R, L, C)
            tl[:R, :L, 2 * C:] = tvv.reshape(R, L, C)
        else:
            c[:, :n0, :2 * C] = torch.cat([kk, vv], dim=-1).reshape(B, n0, 2 * C)
            tl[:R, :L, :2 * C] = torch.cat([tkk, tvv], dim=-1).reshape(R, L, 2 * C)
        caches.append(c.view(B * T, kv_ld).to(DEV))
        tails.append(tl.view((R + 1) * cap, t_ld).to(DEV))
    return dict(q=qbuf[:, qo:], q_ld=q_ld, k=[c[:, ko:] for c in caches], v=[c[:, vo:] for c in caches], kv_ld=kv_ld,
                kv_hs=kv_hs, tk=[x[:, ko:] for x in tails], tv=[x[:, vo:] for x in tails], t_ld=t_ld, cap=cap,
                keep=[qbuf] + caches + tails)


def _launch(layout, q, ks, vs, tks, tvs, n0, t, T):
    """One mmt_op_attention_decode_fanout call; checks the return code, the output's pad columns and the guard
    sample's row. Returns the output bf16 [B, S, H, hs] on the CPU."""
    B, S, H, hs = q.shape
    C, R, ns = H * hs, B * S, len(ks)
    p = _pack(layout, q, ks, vs, tks, tvs, n0, t, T)
    o = torch.full((R + 1, C + O_PAD), SENTINEL, dtype=BF, device=DEV)
    arr = lambda xs: (ctypes.c_void_p * ns)(*[x.data_ptr() for x in xs])  # noqa: E731
    rc = ML.lib().mmt_op_attention_decode_fanout(ML.stream_ptr(), B, S, n0, t, T, H, hs, ns, ML.ptr(p["q"]), p["q_ld"],
                                                 arr(p["k"]), arr(p["v"]), p["kv_ld"], p["kv_hs"], arr(p["tk"]),
                                                 arr(p["tv"]), p["t_ld"], p["cap"], ML.ptr(o), C + O_PAD)
    assert rc == 0, rc
    torch.cuda.synchronize()
    o = o.cpu()
    assert (o[:, C:] == SENTINEL).all(), "the output's pad columns were written"
    assert (o[R] == SENTINEL).all(), "the row after the last sample was written"
    return o[:R, :C].reshape(B, S, H, hs)


def _inputs(kind, B, S, H, T, hs, ns, cap, n0, t, seed, **kw):
    scale = hs ** -0.5
    if kind == "random":
        return F.build_random(B, S, H, T, hs, ns, cap, seed)
    if kind == "needle":
        return F.build_needle(B, S, H, T, hs, ns, cap, n0, t, scale, seed)[:5]
    if kind == "shifted":
        return F.build_shifted(B, S, H, T, hs, ns, cap, scale, seed, **kw)
    assert kind == "flat"
    return F.build_flat(B, S, H, T, hs, ns, cap, seed)


class _Worst:
    """The largest bound ratio of a test, printed at its end; the first element outside the bound fails it."""

    def __init__(self, name):
        self.name, self.ratio, self.where = name, 0.0, None

    def case(self, kind, layout, B, S, H, n0, t, hs, ns, T=None, seed=0, **kw):
        T = t + 2 if T is None else T
        cap = t - n0 + 2
        q, ks, vs, tks, tvs = _inputs(kind, B, S, H, T, hs, ns, cap, n0, t, seed, **kw)
        out = _launch(layout, q, ks, vs, tks, tvs, n0, t, T)
        ref, A = F.fanout_attention_ref(q, ks, vs, tks, tvs, n0, t, hs ** -0.5)
        r, at = F.worst_ratio(out, ref, A, t + 1, n0)
        what = f"{kind} {layout} B {B} S {S} H {H} T {T} n0 {n0} t {t} hs {hs} streams {ns} {kw or ''}"
        if r > self.ratio:
            self.ratio, self.where = r, (what, at)
        assert r <= 1.0, (f"{what}: |out - ref| / tol = {r:.3f} at (b, s, h, d) = {at}: out {float(out[at]):.6g} "
                          f"ref {float(ref[at]):.6g}")
        if kind == "flat":
            want = F.flat_expected(vs, tvs, n0, t)
            same = out.view(torch.int16) == want.view(torch.int16)
            assert same.all(), (f"{what}: {int((~same).sum())} elements differ from bf16(mean), first at "
                                f"{tuple(int(x) for x in (~same).nonzero()[0])}")
        return r

    def done(self):
        print(f"fan-out kernel, {self.name}: largest |out - ref| / tol = {self.ratio:.3f} at {self.where}")


SAMPLES = (1, G - 1, G, G + 1, 2 * G + 3)
# (n0, pos): the smallest window, a one-row prefix with a tail, a tail of one row, across the 256-key line, and
# either side of a 64-key tile boundary in the prefix
WINDOWS = ((1, 1), (1, 9), (7, 7), (250, 263), (63, 70), (64, 70), (65, 70))


@pytest.mark.parametrize("kind", ["needle", "random"])
@pytest.mark.parametrize("hs", HEAD_SIZES)
def test_kernel_shapes(hs, kind):
    """Every head size, S around the group of 16 samples, B = 3 (where r / S matters) and B = 1, both layouts."""
    w = _Worst(f"shapes {kind} hs {hs}")
    for S in SAMPLES:
        for B in (1, 3):
            for n0, t in WINDOWS[:4] if kind == "needle" else WINDOWS:
                w.case(kind, "self", B, S, 2, n0, t, hs, 1, seed=hs + S + t)
                w.case(kind, "cross", B, S, 2, n0, t, hs, 2, seed=hs + S + t)
    w.done()


def test_kernel_largest_block():
    """T = 4096 at hs 64: 63 prefix tiles, a tail across a tile boundary (91 rows), a short last group."""
    w = _Worst("largest block")
    for layout in LAYOUTS:
        w.case("needle", layout, 1, G + 1, 1, 4000, 4090, 64, 1, T=4096, seed=5)
    w.done()


def test_kernel_stream_count():
    w = _Worst("stream count")
    for ns in (7, 8):
        w.case("needle", "cross", 2, 3, 2, 20, 37, 32, ns, seed=ns)
    w.done()


@pytest.mark.parametrize("hs", [8, 32, 64])
def test_kernel_exact_count_bit_equality(hs):
    """Flat inputs, n a power of two spanning prefix and tail: bf16(mean) bit for bit."""
    w = _Worst(f"flat hs {hs}")
    for n0, t in ((1, 1), (2, 3), (48, 63), (64, 127), (200, 255), (100, 255)):
        for ns, layout in ((1, "self"), (3, "cross")):
            w.case("flat", layout, 2, G + 1, 2, n0, t, hs, ns, seed=t + ns)
    w.done()


@pytest.mark.parametrize("shift", [60.0, 100.0])
def test_kernel_rescale_both_directions(shift):
    """Scores near +-shift: even samples have the large ones in the prefix only (the tail underflows against the
    running maximum), odd samples in the tail only (the first tail tile rescales the whole prefix away)."""
    w = _Worst(f"shifted {shift:g}")
    for n0, t in ((7, 9), (70, 140)):
        for hs in (32, 64):
            for ns, layout in ((1, "self"), (2, "cross")):
                w.case("shifted", layout, 2, G + 2, 2, n0, t, hs, ns, seed=t + hs + ns, shift=shift)
    w.done()


@pytest.mark.parametrize("hs", [16, 64])
def test_kernel_sample_independence_and_determinism(hs):
    """Sample s of a launch of S equals, bit for bit, the same sample launched alone (S = 1, its own tail); two
    identical launches are bit-equal."""
    B, S, H, n0, t, ns = 2, 2 * G + 3, 2, 70, 140, 2
    T, cap = t + 2, t - n0 + 2
    q, ks, vs, tks, tvs = F.build_random(B, S, H, T, hs, ns, cap, seed=hs)
    a = _launch("cross", q, ks, vs, tks, tvs, n0, t, T)
    b = _launch("cross", q, ks, vs, tks, tvs, n0, t, T)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    for s in (0, 5, G - 1, G, 2 * G + 2):
        one = _launch("cross", q[:, s:s + 1], ks, vs, [x[:, s:s + 1] for x in tks], [x[:, s:s + 1] for x in tvs], n0, t, T)
        assert torch.equal(one.view(torch.int16), a[:, s:s + 1].view(torch.int16)), s


def test_kernel_entry_refuses_before_any_launch():
    B, S, H, T, hs, n0, t, cap = 2, 3, 2, 16, 8, 4, 5, 4
    C, R = H * hs, 6
    L = ML.lib()
    q = torch.randn(R, 3 * C, device=DEV).to(BF)
    cache = torch.randn(B * T, 3 * C, device=DEV).to(BF)
    tail = torch.randn(R * cap, 3 * C, device=DEV).to(BF)
    o = torch.full((R, C + O_PAD), SENTINEL, dtype=BF, device=DEV)
    nine = lambda x: (ctypes.c_void_p * 9)(*[x.data_ptr()] * 9)  # noqa: E731
    kp, vp, tkp, tvp = nine(cache), nine(cache[:, 2 * C:]), nine(tail), nine(tail[:, 2 * C:])
    null = ctypes.c_void_p(0)

    def call(B=B, S=S, n0=n0, t=t, T=T, H=H, hs=hs, ns=1, qp=ML.ptr(q[:, C:]), q_ld=3 * C, k=kp, v=vp, kv_ld=3 * C,
             kv_hs=hs, tk=tkp, tv=tvp, t_ld=3 * C, rows=cap, op=ML.ptr(o), untouched=True):
        rc = L.mmt_op_attention_decode_fanout(ML.stream_ptr(), B, S, n0, t, T, H, hs, ns, qp, q_ld, k, v, kv_ld, kv_hs,
                                              tk, tv, t_ld, rows, op, C + O_PAD)
        torch.cuda.synchronize()
        assert not untouched or (o == SENTINEL).all(), "a refused call wrote the output"
        return rc

    assert call(hs=12, kv_hs=8) == -2  # MMT_ERR_UNSUPPORTED
    for kw in (dict(t=T), dict(t=-1), dict(ns=0), dict(ns=9), dict(kv_ld=3 * C + 4), dict(q_ld=3 * C + 4),
               dict(kv_hs=hs + 4), dict(t_ld=3 * C + 4), dict(B=0), dict(H=0), dict(S=0), dict(S=-2), dict(n0=0),
               dict(n0=t + 1), dict(rows=0), dict(rows=1), dict(qp=null), dict(op=null), dict(k=None), dict(tk=None),
               dict(tv=None)):
        assert call(**kw) == -1, kw  # MMT_ERR_INVALID
    assert call(untouched=False) == 0  # and the same arguments unmodified run
    assert (o[:, C:] == SENTINEL).all() and torch.isfinite(o[:, :C].float()).all()


# --------------------------------------------------------------------------------------- engine level
V3, CROSS3 = [37, 5, 11], [True, False, False]


def build(meta, sd, dropout=0.0):
    config_utils._config_cache = {"n_embd": meta["n_embd"], "n_head": meta["n_head"], "n_layer": meta["n_layer"],
                                  "block_size": meta["block_size"], "dropout": dropout, "device": "cuda",
                                  "batch_size": meta["B"], "eval_iters": 1}
    import model as mmt_model
    params = []
    for i, v in enumerate(meta["V"]):
        p = [None] * 12
        p[8] = meta["cross"][i]
        params.append(p)
    m = mmt_model.MultimodalTransformer(len(meta["V"]), meta["V"], params).to("cuda")
    full = dict(sd)
    T = meta["block_size"]
    for k in meta["state_dict_keys"]:
        if k.endswith("tril"):
            full[k] = torch.tril(torch.ones(T, T))
    m.load_state_dict(full, strict=True)
    return m


def _model(hs, H, L, T, B, seed):
    """The recipe of test_gpu_decode.py: 3 modalities, cross-attention on modality 0, perturbed biases and
    LayerNorms."""
    import mmt_oracle as O
    C = H * hs
    cfg = O.OracleConfig(C, H, L, T, V3, CROSS3)
    g = torch.Generator().manual_seed(seed)
    sd = O.init_params(cfg, g)
    for k in sd:
        if k.endswith("bias") or "ln" in k or "norm" in k:
            sd[k] = sd[k] + 0.05 * torch.randn(sd[k].shape, generator=g)
    tril = [f"blocks.{l}.{kind}.{i}.heads.{h}.tril" for l in range(L) for i in range(len(V3))
            for kind in ("sa_layers", "cross_attention_layers") for h in range(H)
            if kind == "sa_layers" or CROSS3[i]]
    meta = {"n_embd": C, "n_head": H, "n_layer": L, "block_size": T, "B": B, "V": V3, "cross": CROSS3,
            "state_dict_keys": list(sd.keys()) + tril}
    m = build(meta, sd)
    m.eval()
    idx = [torch.randint(0, v, (B, T), generator=g) for v in V3]
    return m, sd, cfg, idx, g


def _fan_sequences(idx, S, n0, g):
    """[B*S, T] per modality: row b*S + s shares prompt b's first n0 tokens and has its own after."""
    import model as mmt_model
    rows = mmt_model.tile_prompts(idx, S)
    for i, r in enumerate(rows):
        r[:, n0:] = torch.randint(0, V3[i], r[:, n0:].shape, generator=g)
    return rows


# name: hs, H, L, T, B, S, n0 (prefill length; positions n0..T-1 are decoded for B*S rows)
ENGINE_CASES = {
    "long_block_hs32": (32, 2, 1, 320, 2, 3, 250),
    "long_block_hs64": (64, 1, 1, 320, 1, 5, 250),
    "one_sample": (32, 2, 2, 40, 1, 1, 7),
    "rows_above_a_gemm_tile": (16, 2, 1, 16, 2, 70, 5),
    "c256_hs32": (32, 8, 1, 48, 2, 17, 20),
}
FACTOR = 2.0  # as test_gpu_decode.py: per position at most twice the full forward's own worst deviation


def _check_logits(name, dec, full, ref, n0, T):
    """dec[t - n0][i]: [R, V_i] at positions n0..T-1; the three criteria of test_engine_decode_per_position."""
    for i in range(len(V3)):
        got = torch.stack([d[i] for d in dec], dim=1)  # [R, T-n0, V]
        r_full, r_ref = rel(got, full[i][:, n0:T]), rel(got, ref[i][:, n0:T])
        e_full = max(rel(full[i][:, t], ref[i][:, t]) for t in range(T))
        per = [rel(dec[t - n0][i], ref[i][:, t]) for t in range(n0, T)]
        e_dec = max(per)
        t_worst = n0 + per.index(e_dec)
        print(f"fan-out engine, {name}, modality {i}: stacked rel vs full {r_full:.2e}, vs oracle {r_ref:.2e}; per "
              f"position max rel vs oracle {e_dec:.2e} (t = {t_worst}), full forward's e_full {e_full:.2e}, "
              f"ratio {e_dec / e_full:.2f}")
        assert r_full < 1e-2, (name, i, r_full)
        assert r_ref < 2e-2, (name, i, r_ref)
        assert e_dec <= FACTOR * e_full, (name, i, t_worst, e_dec, e_full)


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_engine_fanout_teacher_forcing(name):
    import mmt_oracle as O
    hs, H, L, T, B, S, n0 = ENGINE_CASES[name]
    m, sd, cfg, idx, g = _model(hs, H, L, T, B, seed=2000 + hs + T + B + S)
    rows = _fan_sequences(idx, S, n0, g)
    seq = [r.cuda() for r in rows]
    with torch.no_grad():
        full, _ = m(seq)
        full = [f.cpu() for f in full]
        m([t[:, :n0].cuda() for t in idx])
        dec = [[d.cpu() for d in m._decode_fanout_step([s[:, t] for s in seq], t, S, n0, T - n0)]
               for t in range(n0, T)]
    ref, _ = O.forward(sd, cfg, rows)
    _check_logits(name, dec, full, ref, n0, T)


def test_engine_fanout_leaves_the_workspace_untouched():
    hs, H, L, T, B, S, n0 = 32, 2, 2, 40, 2, 5, 7
    m, sd, cfg, idx, g = _model(hs, H, L, T, B, seed=91)
    seq = [r.cuda() for r in _fan_sequences(idx, S, n0, g)]
    at_n0 = [t[:, n0].cuda() for t in idx]
    with torch.no_grad():
        m([t[:, :n0].cuda() for t in idx])
        before = [x.clone() for x in m._decode_step(at_n0, n0)]
        for t in range(n0, T):
            m._decode_fanout_step([s[:, t] for s in seq], t, S, n0, T - n0)
        after = [x.clone() for x in m._decode_step(at_n0, n0)]
    for i in range(len(V3)):
        assert torch.equal(before[i], after[i]), i


def test_engine_step_refusals_leave_the_logits_alone():
    hs, H, L, T, B, S, n0 = 16, 2, 1, 16, 2, 3, 5
    m, sd, cfg, idx, g = _model(hs, H, L, T, B, seed=17)
    Lb = ML.lib()
    R, N = B * S, T - n0
    tok = [torch.zeros(R, dtype=torch.long, device=DEV) for _ in V3]
    logits = [torch.full((R, v), SENTINEL, dtype=torch.float32, device=DEV) for v in V3]
    fan = torch.empty(Lb.mmt_fanout_bytes(m._ctx, B, S, N), dtype=torch.uint8, device=DEV)

    def step(pos, B=B, S=S, n0=n0, N=N, ws=None):
        ws = m._ws if ws is None else ws
        rc = Lb.mmt_decode_fanout_step(m._ctx, ML.stream_ptr(), B, S, n0, N, pos, ML.ptr_array(tok), ML.ptr(m.flat_params),
                                       ML.ptr_array(logits), ML.ptr(ws), ML.ptr(fan))
        torch.cuda.synchronize()
        return rc

    untouched = lambda: all((x == SENTINEL).all() for x in logits)  # noqa: E731
    assert step(n0, ws=fan) == -4 and untouched()  # MMT_ERR_STATE: no prefill yet
    with torch.no_grad():
        m([t[:, :n0].cuda() for t in idx])
    assert step(n0 + 1) == -4 and untouched()  # a run starts at n0
    for kw in (dict(pos=n0 - 1), dict(pos=n0 + N), dict(pos=n0, S=0), dict(pos=n0, S=-1), dict(pos=n0, n0=0),
               dict(pos=n0, N=0), dict(pos=n0, N=T - n0 + 1)):
        assert step(**kw) == -1 and untouched(), kw  # MMT_ERR_INVALID
    assert step(n0, B=B + 1) == -4 and untouched()  # not the prefill's batch
    assert step(n0) == 0 and not untouched()
    for x in logits:
        x.fill_(SENTINEL)
    assert step(n0 + 2) == -4 and untouched()  # skipped n0 + 1
    assert step(n0 + 1, S=S + 1) == -4 and untouched()  # another sample count mid-run
    assert step(n0 + 1) == 0 and torch.isfinite(logits[0]).all()
    with torch.no_grad():
        m([t[:, :n0].cuda() for t in idx])
    for x in logits:
        x.fill_(SENTINEL)
    assert step(n0 + 2) == -4 and untouched()  # a new prefill ended the run


def test_generate_num_samples_keying_logits_and_paths():
    import mmt_oracle as O
    import mmt_sample as MS
    hs, H, L, T, B, S, n0, N, gmod, seed = 32, 2, 2, 40, 2, 5, 7, 12, 0, 1234
    m, sd, cfg, idx, g = _model(hs, H, L, T, B, seed=55)
    prompts = [t[:, :n0].cuda() for t in idx]
    seen = {}
    hook = lambda n, lg: seen.__setitem__(n, lg.clone())  # noqa: E731
    kw = dict(max_new_tokens=N, modality_to_generate=gmod, temperature=0.9, top_k=5, seed=seed, return_logprobs=True)
    seqs, lp = m.generate(prompts, logits_hook=hook, num_samples=S, **kw)
    assert m.last_generate_path == "fanout"
    R = B * S
    assert all(tuple(s.shape) == (R, n0 + N) for s in seqs) and tuple(lp.shape) == (R, N)
    assert sorted(seen) == list(range(n0, n0 + N)) and all(tuple(v.shape) == (R, V3[gmod]) for v in seen.values())
    for i in range(len(V3)):  # the prompts, tiled, and the other modalities' pad with their last token
        assert torch.equal(seqs[i][:, :n0], prompts[i].repeat_interleave(S, 0))
        if i != gmod:
            assert (seqs[i][:, n0:] == seqs[i][:, n0 - 1:n0]).all()
    # row and position keying, buffer wiring: re-sampling the captured logits reproduces tokens and log-probabilities
    for n in range(n0, n0 + N):
        tok, l = MS.sample(seen[n], temperature=0.9, top_k=5, seed=seed, row0=0, pos=n, return_logprobs=True)
        assert torch.equal(tok, seqs[gmod][:, n]), n
        assert torch.equal(l, lp[:, n - n0]), n
    # the captured logits against a full forward of the returned sequences, and the oracle
    Tn = n0 + N
    with torch.no_grad():
        full, _ = m(seqs)
    full = [f.cpu() for f in full]
    ref, _ = O.forward(sd, cfg, [torch.nn.functional.pad(s.cpu(), (0, T - Tn)) for s in seqs])
    got = torch.stack([seen[n].cpu() for n in range(n0, Tn)], dim=1)  # logits at positions n0-1 .. Tn-2
    fg, rg = full[gmod][:, n0 - 1:Tn - 1], ref[gmod][:, n0 - 1:Tn - 1]
    e_full = max(rel(full[gmod][:, t], ref[gmod][:, t]) for t in range(Tn))
    per = [rel(got[:, j], rg[:, j]) for j in range(N)]
    print(f"generate fan-out: stacked rel vs full {rel(got, fg):.2e}, vs oracle {rel(got, rg):.2e}, per position max "
          f"{max(per):.2e}, e_full {e_full:.2e}")
    assert rel(got, fg) < 1e-2 and rel(got, rg) < 2e-2 and max(per) <= FACTOR * e_full
    # use_cache=False: tiled, the same shapes
    seqs2, lp2 = m.generate(prompts, use_cache=False, num_samples=S, **kw)
    assert m.last_generate_path == "tiled"
    assert all(tuple(s.shape) == (R, n0 + N) for s in seqs2) and tuple(lp2.shape) == (R, N)


def test_generate_fallbacks_and_default():
    hs, H, L, T, B, S, n0 = 32, 2, 1, 24, 2, 3, 5
    m, sd, cfg, idx, g = _model(hs, H, L, T, B, seed=56)
    prompts = [t[:, :n0].cuda() for t in idx]
    kw = dict(modality_to_generate=0, temperature=0.8, seed=9, return_logprobs=True)
    # across block_size: tiled, and exactly the caller-tiled call
    a, la = m.generate(prompts, max_new_tokens=T - n0 + 2, num_samples=S, **kw)
    assert m.last_generate_path == "tiled"
    b, lb = m.generate([p.repeat_interleave(S, 0) for p in prompts], max_new_tokens=T - n0 + 2, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(la, lb)
    # prompts of unequal lengths (here all at least a block long, which the re-forward's crop equalises): tiled
    e, _ = m.generate([torch.cat([p, p, p, p, p[:, :4 + (i == 1)]], dim=1) for i, p in enumerate(prompts)],
                      max_new_tokens=2, num_samples=S, **kw)
    assert m.last_generate_path == "tiled" and e[0].shape[0] == B * S
    # num_samples=None is the call without the keyword
    c, lc = m.generate(prompts, max_new_tokens=6, num_samples=None, **kw)
    d, ld = m.generate(prompts, max_new_tokens=6, **kw)
    assert all(torch.equal(x, y) for x, y in zip(c, d)) and torch.equal(lc, ld)
    with pytest.raises(ValueError):
        m.generate(prompts, max_new_tokens=2, num_samples=S, sample_fn=lambda p: p.argmax(-1, keepdim=True))
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            m.generate(prompts, max_new_tokens=2, num_samples=bad)


def test_generate_greedy_fanout_equals_tiled():
    """Peaked output heads (the x60 recipe of test_generate_batch_1_cache_matches_reforward), temperature 0: the
    fan-out tokens equal the tiled ones, and all samples of a prompt coincide."""
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    sd = dict(sd)
    for k in list(sd):
        if k.startswith("post_block.soft_score_layers.") and k.endswith(".2.weight"):
            sd[k] = sd[k] * 60.0
    m = build(meta, sd)
    m.eval()
    T, S = meta["block_size"], 5
    start = [t[:2, :5].cuda() for t in idx]
    a = m.generate(start, max_new_tokens=T - 5, modality_to_generate=2, temperature=0, num_samples=S)
    assert m.last_generate_path == "fanout"
    b = m.generate(start, max_new_tokens=T - 5, modality_to_generate=2, temperature=0, num_samples=S, use_cache=False)
    assert m.last_generate_path == "tiled"
    for i in range(cfg.M):
        assert tuple(a[i].shape) == (2 * S, T) and torch.equal(a[i], b[i]), i
        assert torch.equal(a[i][0::S].repeat_interleave(S, 0), a[i]), i
