"""The KV-cache decode path on the GPU.

Kernel level: attn_decode_kernel<HS> through mmt_op_attention_decode against the fp64 reference of
tests/decode_ref.py, every element under its derived bound tol (never a norm), in the engine's two cache
layouts. Every cache row above t, K and V alike, and every pad column is NaN, so a kernel that reads one
returns NaN; the output has 8 pad columns of a sentinel that must survive. The flat inputs must come out bit
for bit. tests/test_decode_ref_cpu.py shows that a dropped key, a window one row too long and swapped streams
leave the bound on these inputs.

Engine level: mmt_decode_step at the shapes the model tests never reach (block above 256, B = 1, from
position 1, more rows than a GEMM tile, C = 256), against the full forward and the CPU oracle under the
project's whole-tensor bounds and per decoded position.
"""
import ctypes

import pytest
import torch

import decode_ref as R
import mmt_lib as ML
from golden_io import model_fixture
from test_gpu_model import build, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
SENTINEL = -77.0  # exact in bf16
O_PAD = 8


# --------------------------------------------------------------------------------------- kernel level
def _rows(x, n):
    """[B, H, T, hs] -> [B, n, H, hs]: rows 0..n-1 in cache order."""
    return x[:, :, :n].permute(0, 2, 1, 3)


def _pack(layout, q, ks, vs, t, T):
    """The canonical tensors in one of the engine's layouts, on the device, NaN wherever the kernel must not
    read. Returns (q pointer tensor, q_ld, K tensors, V tensors, kv_ld, kv_hstride, keep-alive list)."""
    B, H, hs = q.shape
    C, n = H * hs, t + 1
    caches, kt, vt = [], [], []
    if layout == "self":
        # the step's compact [B, 3C] K|Q|V rows; the forward's [B*T, 3C] rows as the cache
        qbuf = torch.full((B, 3 * C), NAN, dtype=BF)
        qbuf[:, C:2 * C] = q.reshape(B, C)
        qbuf = qbuf.to(DEV)
        qt, q_ld, kv_ld, kv_hs = qbuf[:, C:], 3 * C, 3 * C, hs
        for k, v in zip(ks, vs):
            c = torch.full((B, T, 3 * C), NAN, dtype=BF)
            c[:, :n, :C] = _rows(k, n).reshape(B, n, C)
            c[:, :n, 2 * C:] = _rows(v, n).reshape(B, n, C)
            c = c.view(B * T, 3 * C).to(DEV)
            caches.append(c)
            kt.append(c)
            vt.append(c[:, 2 * C:])
    else:
        # cross-attention: q [B, C] (here with 8 pad columns), per stream [B*T, 2C (+ 8 pad)] rows, per head K|V
        q_ld, kv_ld, kv_hs = C + 8, 2 * C + 8, 2 * hs
        qbuf = torch.full((B, q_ld), NAN, dtype=BF)
        qbuf[:, :C] = q.reshape(B, C)
        qbuf = qbuf.to(DEV)
        qt = qbuf
        for k, v in zip(ks, vs):
            c = torch.full((B, T, kv_ld), NAN, dtype=BF)
            c[:, :n, :2 * C] = torch.cat([_rows(k, n), _rows(v, n)], dim=-1).reshape(B, n, 2 * C)
            c = c.view(B * T, kv_ld).to(DEV)
            caches.append(c)
            kt.append(c)
            vt.append(c[:, hs:])
    return qt, q_ld, kt, vt, kv_ld, kv_hs, [qbuf] + caches


def _launch(layout, q, ks, vs, t, T):
    """One mmt_op_attention_decode call; checks the return code and the output's pad columns.
    Returns the output bf16 [B, H, hs] on the CPU."""
    B, H, hs = q.shape
    C, ns = H * hs, len(ks)
    qt, q_ld, kt, vt, kv_ld, kv_hs, keep = _pack(layout, q, ks, vs, t, T)
    o = torch.full((B, C + O_PAD), SENTINEL, dtype=BF, device=DEV)
    kp = (ctypes.c_void_p * ns)(*[x.data_ptr() for x in kt])
    vp = (ctypes.c_void_p * ns)(*[x.data_ptr() for x in vt])
    rc = ML.lib().mmt_op_attention_decode(ML.stream_ptr(), B, t, T, H, hs, ns, ML.ptr(qt), q_ld, kp, vp, kv_ld, kv_hs,
                                          ML.ptr(o), C + O_PAD)
    assert rc == 0, rc
    torch.cuda.synchronize()
    o = o.cpu()
    assert (o[:, C:] == SENTINEL).all(), "the output's pad columns were written"
    del keep
    return o[:, :C].reshape(B, H, hs)


def _inputs(kind, B, H, T, t, hs, ns, seed, **kw):
    scale = hs ** -0.5
    if kind == "random":
        return R.build_random(B, H, T, hs, ns, seed)
    if kind == "needle":
        return R.build_needle(B, H, T, hs, ns, t, scale, seed, **kw)[:3]
    if kind == "shifted":
        return R.build_shifted(B, H, T, hs, ns, scale, seed, **kw)
    assert kind == "flat"
    return R.build_flat(B, H, T, hs, ns, seed)


class _Worst:
    """The largest bound ratio of a test, printed at its end; the first element outside the bound fails it."""

    def __init__(self, name):
        self.name, self.ratio, self.where = name, 0.0, None

    def case(self, kind, layout, B, H, T, t, hs, ns, seed=0, **kw):
        q, ks, vs = _inputs(kind, B, H, T, t, hs, ns, seed, **kw)
        out = _launch(layout, q, ks, vs, t, T)
        ref, A = R.decode_attention_ref(q, ks, vs, t, hs ** -0.5)
        r, at = R.worst_ratio(out, ref, A, t + 1)
        what = f"{kind} {layout} B {B} H {H} T {T} hs {hs} streams {ns} {kw or ''}"
        if r > self.ratio:
            self.ratio, self.where = r, (what, t + 1, at)
        assert r <= 1.0, (f"{what}: |out - ref| / tol = {r:.3f} at (b, h, d) = {at}, n = {t + 1}: "
                          f"out {float(out[at]):.6g} ref {float(ref[at]):.6g}")
        if kind == "flat":
            want = R.flat_expected(vs, t)
            same = out.view(torch.int16) == want.view(torch.int16)
            assert same.all(), (f"{what}, n = {t + 1}: {int((~same).sum())} elements differ from bf16(mean), first at "
                                f"{tuple(int(x) for x in (~same).nonzero()[0])}")
        return r

    def done(self):
        print(f"decode kernel, {self.name}: largest |out - ref| / tol = {self.ratio:.3f} at {self.where}")


LAYOUTS = ("self", "cross")


@pytest.mark.parametrize("kind", ["random", "needle"])
@pytest.mark.parametrize("hs", R.HEAD_SIZES)
def test_kernel_low_positions(hs, kind):
    """n = 1..5 of a block of 8: most of the 256 threads and up to three of the four value groups have no key."""
    w = _Worst(f"low positions {kind} hs {hs}")
    for B in (1, 3):
        for H in (1, 3):
            for t in (0, 1, 2, 3, 4):
                w.case(kind, "self", B, H, 8, t, hs, 1, seed=hs + t)
                w.case(kind, "cross", B, H, 8, t, hs, 2, seed=hs + t)
    w.done()


@pytest.mark.parametrize("kind", ["needle", "random"])
@pytest.mark.parametrize("hs", [8, 32, 64])
def test_kernel_second_trip_of_the_strided_loops(hs, kind):
    """n = 255 .. 258 and 320 around the 256 threads of the score loops: exactly one trip, then a second one."""
    w = _Worst(f"second trip {kind} hs {hs}")
    for t in (254, 255, 256, 257, 319):
        for ns in (1, 3):
            for layout in LAYOUTS:
                w.case(kind, layout, 2, 2, 320, t, hs, ns, seed=t + ns)
    w.done()


def test_kernel_many_trips_score_row_sized_from_T():
    w = _Worst("many trips")
    for t in (1023, 511):
        for hs in (32, 64):
            for layout in LAYOUTS:
                w.case("needle", layout, 1, 2, 1024, t, hs, 1, seed=t + hs)
    w.done()


def test_kernel_largest_block():
    """T = 4096 (the f_t4096 configuration's block): 16 trips; the needle at the last row, at the first row of
    the last group of four and just past the first trip."""
    w = _Worst("largest block")
    for layout in LAYOUTS:
        for rot in (1, 6, 4):
            w.case("needle", layout, 1, 1, 4096, 4095, 64, 1, seed=rot, rot=rot)
        w.case("flat", layout, 1, 1, 4096, 4095, 64, 1)
    w.done()


def test_kernel_stream_count():
    """7 and 8 streams (MMT_MAX_STREAMS) summed into one output, the cross layout."""
    w = _Worst("stream count")
    for hs in (32, 24):
        for ns in (7, 8):
            w.case("needle", "cross", 2, 2, 40, 37, hs, ns, seed=ns)
    w.done()


def test_kernel_odd_block_window_shorter_than_block():
    w = _Worst("T odd, T != n")
    for t in (36, 17):
        for hs in (16, 48):
            for ns in (1, 2):
                for layout in LAYOUTS:
                    w.case("random", layout, 3, 3, 37, t, hs, ns, seed=t + hs + ns)
    w.done()


@pytest.mark.parametrize("hs", [8, 32, 64])
def test_kernel_exact_count_bit_equality(hs):
    """Flat inputs: the output is bf16(mean) bit for bit, which a window of n - 1 or n + 1 keys cannot give."""
    w = _Worst(f"flat hs {hs}")
    for t in (0, 1, 3, 255):
        for ns in (1, 3):
            for layout in LAYOUTS:
                w.case("flat", layout, 2, 2, 320, t, hs, ns, seed=t + ns)
    w.done()


def test_kernel_exact_count_longer_rows_bit_equality():
    w = _Worst("flat T 1024")
    for t in (511, 1023):
        for hs in (32, 64):
            for ns in (1, 3):
                for layout in LAYOUTS:
                    w.case("flat", layout, 1, 2, 1024, t, hs, ns, seed=t + ns)
    w.done()


@pytest.mark.parametrize("shift", [60.0, 100.0])
def test_kernel_max_subtraction(shift):
    """All scaled scores of a head near +shift or near -shift. exp(+-60) is still a normal fp32 number, so it
    is the shift of 100 that a kernel without the max subtraction fails (tests/test_decode_ref_cpu.py)."""
    w = _Worst(f"shifted {shift:g}")
    for t in (63, 5):
        for hs in (32, 64):
            for ns in (1, 2):
                for layout in LAYOUTS:
                    w.case("shifted", layout, 2, 2, 64, t, hs, ns, seed=t + hs + ns, shift=shift)
    w.done()


def test_kernel_entry_refuses_before_any_launch():
    B, H, T, hs, t = 2, 2, 16, 8, 5
    C = H * hs
    L = ML.lib()
    q = torch.randn(B, 3 * C, device=DEV).to(BF)
    cache = torch.randn(B * T, 3 * C, device=DEV).to(BF)
    o = torch.full((B, C + O_PAD), SENTINEL, dtype=BF, device=DEV)
    kp = (ctypes.c_void_p * 9)(*[cache.data_ptr()] * 9)
    vp = (ctypes.c_void_p * 9)(*[cache[:, 2 * C:].data_ptr()] * 9)

    def call(t=t, T=T, hs=hs, ns=1, kv_ld=3 * C, q_ld=3 * C, kv_hs=None, B=B, H=H):
        rc = L.mmt_op_attention_decode(ML.stream_ptr(), B, t, T, H, hs, ns, ML.ptr(q[:, C:]), q_ld, kp, vp, kv_ld,
                                       hs if kv_hs is None else kv_hs, ML.ptr(o), C + O_PAD)
        torch.cuda.synchronize()
        assert (o == SENTINEL).all(), "a refused call wrote the output"
        return rc

    assert call(hs=12) == -2  # MMT_ERR_UNSUPPORTED
    for kw in (dict(t=T), dict(t=-1), dict(ns=0), dict(ns=9), dict(kv_ld=3 * C + 4), dict(q_ld=3 * C + 4),
               dict(kv_hs=hs + 4), dict(B=0), dict(H=0)):
        assert call(**kw) == -1, kw  # MMT_ERR_INVALID
    null = ctypes.c_void_p(0)
    assert L.mmt_op_attention_decode(ML.stream_ptr(), B, t, T, H, hs, 1, null, 3 * C, kp, vp, 3 * C, hs, ML.ptr(o),
                                     C + O_PAD) == -1
    assert L.mmt_op_attention_decode(ML.stream_ptr(), B, t, T, H, hs, 1, ML.ptr(q[:, C:]), 3 * C, kp, vp, 3 * C, hs, null,
                                     C + O_PAD) == -1
    assert L.mmt_op_attention_decode(ML.stream_ptr(), B, t, T, H, hs, 1, ML.ptr(q[:, C:]), 3 * C, None, vp, 3 * C, hs,
                                     ML.ptr(o), C + O_PAD) == -1
    torch.cuda.synchronize()
    assert (o == SENTINEL).all()
    # and the same arguments unmodified run
    assert L.mmt_op_attention_decode(ML.stream_ptr(), B, t, T, H, hs, 1, ML.ptr(q[:, C:]), 3 * C, kp, vp, 3 * C, hs,
                                     ML.ptr(o), C + O_PAD) == 0
    torch.cuda.synchronize()
    assert (o[:, C:] == SENTINEL).all() and torch.isfinite(o[:, :C].float()).all()


# --------------------------------------------------------------------------------------- engine level
V3, CROSS3 = [37, 5, 11], [True, False, False]


def _model(hs, H, L, T, B, seed):
    """As test_kv_cache_decode_every_head_size: 3 modalities, cross-attention on modality 0, perturbed biases
    and LayerNorms."""
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
    return m, sd, cfg, idx


# name: hs, H, L, T, B, P (prefill length; positions P..T-1 are decoded)
ENGINE_CASES = {
    "long_block_hs32": (32, 2, 1, 320, 2, 250),  # decode across the 256-key boundary, self and cross attention
    "long_block_hs64": (64, 1, 1, 320, 2, 250),
    "batch_1": (32, 2, 2, 40, 1, 7),  # every decode GEMM has M = 1
    "from_position_1": (32, 2, 2, 24, 3, 1),
    "rows_above_a_gemm_tile": (16, 2, 1, 16, 130, 5),
    "c256_hs32": (32, 8, 1, 48, 2, 20),  # the prefill takes the fused out-projection / FFN kernels, decode plain GEMMs
}
# rel(decode_t, oracle_t) <= FACTOR * max_t rel(full_t, oracle_t): the decode step and the full forward are two
# independent bf16 evaluations of one function; the full forward's own deviation from the oracle is the yardstick
# and one more bf16 evaluation may add its share on top
FACTOR = {name: 2.0 for name in ENGINE_CASES}


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_engine_decode_per_position(name):
    import mmt_oracle as O
    hs, H, L, T, B, P = ENGINE_CASES[name]
    m, sd, cfg, idx = _model(hs, H, L, T, B, seed=1000 + hs + T + B)
    seq = [t.cuda() for t in idx]
    with torch.no_grad():
        m([s[:, :P] for s in seq])
        dec = [[d.cpu() for d in m._decode_step([s[:, t] for s in seq], t)] for t in range(P, T)]
        full, _ = m(seq)
    full = [f.cpu() for f in full]
    ref, _ = O.forward(sd, cfg, idx)
    for i in range(len(V3)):
        got = torch.stack([d[i] for d in dec], dim=1)  # [B, T-P, V]
        r_full, r_ref = rel(got, full[i][:, P:T]), rel(got, ref[i][:, P:T])
        e_full = max(rel(full[i][:, t], ref[i][:, t]) for t in range(T))
        per = [rel(dec[t - P][i], ref[i][:, t]) for t in range(P, T)]
        e_dec = max(per)
        t_worst = P + per.index(e_dec)
        print(f"decode engine, {name}, modality {i}: stacked rel vs full {r_full:.2e}, vs oracle {r_ref:.2e}; per position "
              f"max rel vs oracle {e_dec:.2e} (t = {t_worst}), full forward's e_full {e_full:.2e}, "
              f"ratio {e_dec / e_full:.2f}")
        assert r_full < 1e-2, (name, i, r_full)
        assert r_ref < 2e-2, (name, i, r_ref)
        assert e_dec <= FACTOR[name] * e_full, (name, i, t_worst, e_dec, e_full)


def test_engine_append_overwrites_and_prefill_rows_serve_decode():
    """After decoding P..T-1, an eval prefill of the whole sequence rewrites every cache row; decoding T-1
    again then reads rows the prefill kernels wrote where the first pass read rows its own steps appended:
    the same logits within the whole-tensor bound. A second identical step is bit-equal (the append overwrites
    row T-1, nothing accumulates)."""
    hs, H, L, T, B, P = 32, 2, 2, 40, 3, 7
    m, sd, cfg, idx = _model(hs, H, L, T, B, seed=77)
    seq = [t.cuda() for t in idx]
    last = [s[:, T - 1] for s in seq]
    with torch.no_grad():
        m([s[:, :P] for s in seq])
        for t in range(P, T):
            first = m._decode_step([s[:, t] for s in seq], t)
        first = [x.clone() for x in first]
        m(seq)
        again = [x.clone() for x in m._decode_step(last, T - 1)]
        twice = [x.clone() for x in m._decode_step(last, T - 1)]
    for i in range(len(V3)):
        r = rel(again[i], first[i])
        print(f"decode engine, overwrite, modality {i}: rel of T-1 after a full prefill vs after decode steps {r:.2e}")
        assert r < 1e-2, (i, r)
        assert torch.equal(again[i], twice[i]), i


def test_generate_batch_1_cache_matches_reforward():
    """One prompt (what a user calling generate gets): greedy tokens with the KV cache against the re-forward
    per token, on the default path and on the device path at temperature 0; peaked output heads as in
    test_generate_kv_cache_greedy_matches_reforward."""
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    sd = dict(sd)
    for k in list(sd):
        if k.startswith("post_block.soft_score_layers.") and k.endswith(".2.weight"):
            sd[k] = sd[k] * 60.0
    m = build(meta, sd)
    m.eval()
    T = meta["block_size"]
    start = [t[:1, :5].cuda() for t in idx]
    n_new = T + 2 - 5  # two tokens past the block: the cache path hands over to the re-forward
    greedy = lambda probs: probs.argmax(dim=-1, keepdim=True)  # noqa: E731
    a = m.generate(start, max_new_tokens=n_new, modality_to_generate=2, use_cache=True, sample_fn=greedy)
    b = m.generate(start, max_new_tokens=n_new, modality_to_generate=2, use_cache=False, sample_fn=greedy)
    c = m.generate(start, max_new_tokens=n_new, modality_to_generate=2, use_cache=True, temperature=0)
    d = m.generate(start, max_new_tokens=n_new, modality_to_generate=2, use_cache=False, temperature=0)
    for i in range(cfg.M):
        assert tuple(a[i].shape) == (1, T + 2) and tuple(c[i].shape) == (1, T + 2)
        assert torch.equal(a[i], b[i]), i
        assert torch.equal(c[i], d[i]), i
