"""Rolling-window fan-out attention on the GPU: attn_rolling_fanout_kernel<HS> through
mmt_op_attention_rolling_fanout (m tail queries per path in one launch).

Query (r, i), row r*m + i of the compact Q, must be bit-equal to mmt_op_attention_decode_fanout at n0 = p, t = p + i
on the same Q, cache and tails with tail_rows = m (one device function serves both kernels), and within tol_fan of
the fp64 reference of tests/fanout_ref.py. Every cache row at a position >= p, every pad column and the whole tail,
query and output row block of a guard path after row B*S are NaN (the output's: a sentinel that must survive).
"""
import ctypes

import pytest
import torch

import fanout_ref as F
import mmt_lib as ML

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
SENTINEL = -77.0  # exact in bf16
O_PAD = 8

# (hs, H, B, S, p, m, streams)
CASES = [
    (32, 2, 2, 17, 5, 3, 1),    # S crosses a group of 16
    (16, 2, 1, 2, 10, 70, 1),   # tail past one 64-key tile
    (32, 1, 1, 3, 130, 2, 1),   # prefix over three tiles, with a short last tile
    (64, 1, 1, 5, 7, 4, 2),
    (8, 1, 1, 1, 1, 1, 1),
    (32, 2, 1, 3, 9, 5, 8),
]


def _inputs(hs, H, B, S, p, m, ns, seed):
    """Canonical tensors of fanout_ref (build_random) with m queries per path: q bf16 [B, S, m, H, hs]."""
    T = p + m + 1
    _, ks, vs, tks, tvs = F.build_random(B, S, H, T, hs, ns, m, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    q = torch.randn(B, S, m, H, hs, generator=g).to(BF)
    return q, ks, vs, tks, tvs, T


def _pack(q, ks, vs, tks, tvs, p, T):
    """The engine's layouts on the device. One stream: the self-attention layout (K|Q|V rows of 3C, the tails ARE the
    query rows' K and V columns, as mmt_rolling_step has them). More: the cross layout with pad columns."""
    B, S, m, H, hs = q.shape
    C, R, ns = H * hs, B * S, len(ks)
    rows = (R + 1) * m  # one guard path after the last
    if ns == 1:
        q_ld = kv_ld = t_ld = 3 * C
        kv_hs, qo, ko, vo = hs, C, 0, 2 * C
    else:
        q_ld, kv_ld, t_ld = C + 8, 2 * C + 8, 2 * C + 8
        kv_hs, qo, ko, vo = 2 * hs, 0, 0, hs
    qbuf = torch.full((rows, q_ld), NAN, dtype=BF)
    qbuf[:R * m, qo:qo + C] = q.reshape(R * m, C)
    caches, tails = [], []
    for k, v, tk, tv in zip(ks, vs, tks, tvs):
        c = torch.full((B, T, kv_ld), NAN, dtype=BF)
        kk, vv = k[:, :, :p].permute(0, 2, 1, 3), v[:, :, :p].permute(0, 2, 1, 3)  # [B, p, H, hs]
        tkk, tvv = tk.permute(0, 1, 3, 2, 4), tv.permute(0, 1, 3, 2, 4)  # [B, S, m, H, hs]
        if ns == 1:
            c[:, :p, :C] = kk.reshape(B, p, C)
            c[:, :p, 2 * C:] = vv.reshape(B, p, C)
            qbuf[:R * m, :C] = tkk.reshape(R * m, C)
            qbuf[:R * m, 2 * C:] = tvv.reshape(R * m, C)
            tails.append(None)
        else:
            tl = torch.full((rows, t_ld), NAN, dtype=BF)
            c[:, :p, :2 * C] = torch.cat([kk, vv], dim=-1).reshape(B, p, 2 * C)
            tl[:R * m, :2 * C] = torch.cat([tkk, tvv], dim=-1).reshape(R * m, 2 * C)
            tails.append(tl.to(DEV))
        caches.append(c.view(B * T, kv_ld).to(DEV))
    qbuf = qbuf.to(DEV)
    if ns == 1:
        tails = [qbuf]
    return dict(q=qbuf[:, qo:], q_ld=q_ld, k=[c[:, ko:] for c in caches], v=[c[:, vo:] for c in caches], kv_ld=kv_ld,
                kv_hs=kv_hs, tk=[x[:, ko:] for x in tails], tv=[x[:, vo:] for x in tails], t_ld=t_ld,
                keep=[qbuf] + caches + tails)


def _arr(xs):
    return (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])


def _rolling(pk, B, S, p, m, T, H, hs, ns):
    """One mmt_op_attention_rolling_fanout call. Returns the whole output [(R + 1) * m, C + O_PAD] on the CPU."""
    C, R = H * hs, B * S
    o = torch.full(((R + 1) * m, C + O_PAD), SENTINEL, dtype=BF, device=DEV)
    rc = ML.lib().mmt_op_attention_rolling_fanout(ML.stream_ptr(), B, S, p, m, T, H, hs, ns, ML.ptr(pk["q"]), pk["q_ld"],
                                                  _arr(pk["k"]), _arr(pk["v"]), pk["kv_ld"], pk["kv_hs"], _arr(pk["tk"]),
                                                  _arr(pk["tv"]), pk["t_ld"], m, ML.ptr(o), C + O_PAD)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return o.cpu()


def _existing(pk, B, S, p, m, T, H, hs, ns, i):
    """mmt_op_attention_decode_fanout at n0 = p, t = p + i over the same buffers with tail_rows = m: its compact row r
    is query (r, i), so Q and O are passed with a leading dimension of m rows, starting at row i. [R, C] on the CPU."""
    C, R = H * hs, B * S
    o = torch.full(((R + 1) * m, C + O_PAD), SENTINEL, dtype=BF, device=DEV)
    rc = ML.lib().mmt_op_attention_decode_fanout(ML.stream_ptr(), B, S, p, p + i, T, H, hs, ns, ML.ptr(pk["q"][i:]),
                                                 m * pk["q_ld"], _arr(pk["k"]), _arr(pk["v"]), pk["kv_ld"], pk["kv_hs"],
                                                 _arr(pk["tk"]), _arr(pk["tv"]), pk["t_ld"], m, ML.ptr(o[i:]),
                                                 m * (C + O_PAD))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return o.cpu()[i::m][:R, :C]


@pytest.mark.parametrize("hs,H,B,S,p,m,ns", CASES)
def test_kernel_bit_equal_to_the_fanout_kernel_and_within_the_bound(hs, H, B, S, p, m, ns):
    q, ks, vs, tks, tvs, T = _inputs(hs, H, B, S, p, m, ns, seed=hs + S + p + m)
    pk = _pack(q, ks, vs, tks, tvs, p, T)
    C, R = H * hs, B * S
    full = _rolling(pk, B, S, p, m, T, H, hs, ns)
    # guard band: the columns past C and the guard path's m rows keep their sentinel
    assert (full[:, C:] == SENTINEL).all(), "the output's pad columns were written"
    assert (full[R * m:] == SENTINEL).all(), "rows after the last path were written"
    out = full[:R * m, :C].reshape(R, m, C)
    assert torch.isfinite(out.float()).all()
    worst = 0.0
    for i in range(m):
        same = out[:, i].view(torch.int16) == _existing(pk, B, S, p, m, T, H, hs, ns, i).view(torch.int16)
        assert same.all(), (f"tail position {i}: {int((~same).sum())} elements differ from "
                            f"mmt_op_attention_decode_fanout at n0 = {p}, t = {p + i}")
        ref, A = F.fanout_attention_ref(q[:, :, i], ks, vs, tks, tvs, p, p + i, hs ** -0.5)
        r, at = F.worst_ratio(out[:, i].reshape(B, S, H, hs), ref, A, p + i + 1, p)
        assert r <= 1.0, f"tail position {i}: |out - ref| / tol_fan = {r:.3f} at (b, s, h, d) = {at}"
        worst = max(worst, r)
    print(f"rolling kernel hs {hs} H {H} B {B} S {S} p {p} m {m} streams {ns}: largest |out - ref| / tol = {worst:.3f}")


def test_kernel_sample_independence():
    """Changing another sample's tail (and query) changes no bit of this sample's rows."""
    hs, H, B, S, p, m, ns = 32, 2, 2, 17, 70, 5, 2
    q, ks, vs, tks, tvs, T = _inputs(hs, H, B, S, p, m, ns, seed=3)
    C, R = H * hs, B * S
    a = _rolling(_pack(q, ks, vs, tks, tvs, p, T), B, S, p, m, T, H, hs, ns)[:R * m, :C].reshape(B, S, m, C)
    b = _rolling(_pack(q, ks, vs, tks, tvs, p, T), B, S, p, m, T, H, hs, ns)[:R * m, :C].reshape(B, S, m, C)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))  # run to run
    g = torch.Generator().manual_seed(99)
    for s in (0, 15, 16):
        q2 = torch.randn(q.shape, generator=g).to(BF)
        tks2 = [torch.randn(x.shape, generator=g).to(BF) for x in tks]
        tvs2 = [torch.randn(x.shape, generator=g).to(BF) for x in tvs]
        q2[:, s] = q[:, s]
        for x2, x in zip(tks2 + tvs2, tks + tvs):
            x2[:, s] = x[:, s]
        c = _rolling(_pack(q2, ks, vs, tks2, tvs2, p, T), B, S, p, m, T, H, hs, ns)[:R * m, :C].reshape(B, S, m, C)
        assert torch.equal(c[:, s].view(torch.int16), a[:, s].view(torch.int16)), s
        assert not torch.equal(c.view(torch.int16), a.view(torch.int16))


def test_kernel_entry_refuses_before_any_launch():
    """The refusal list of mmt_op_attention_decode_fanout with p for n0 and m for the tail: nothing is written."""
    B, S, H, T, hs, p, m = 2, 3, 2, 16, 8, 4, 3
    C, R = H * hs, 6
    L = ML.lib()
    qkv = torch.randn(R * m, 3 * C, device=DEV).to(BF)
    cache = torch.randn(B * T, 3 * C, device=DEV).to(BF)
    o = torch.full((R * m, C + O_PAD), SENTINEL, dtype=BF, device=DEV)
    nine = lambda x: (ctypes.c_void_p * 9)(*[x.data_ptr()] * 9)  # noqa: E731
    kp, vp, tkp, tvp = nine(cache), nine(cache[:, 2 * C:]), nine(qkv), nine(qkv[:, 2 * C:])
    null = ctypes.c_void_p(0)

    def call(B=B, S=S, p=p, m=m, T=T, H=H, hs=hs, ns=1, qp=ML.ptr(qkv[:, C:]), q_ld=3 * C, k=kp, v=vp, kv_ld=3 * C,
             kv_hs=hs, tk=tkp, tv=tvp, t_ld=3 * C, rows=m, op=ML.ptr(o), untouched=True):
        rc = L.mmt_op_attention_rolling_fanout(ML.stream_ptr(), B, S, p, m, T, H, hs, ns, qp, q_ld, k, v, kv_ld, kv_hs,
                                               tk, tv, t_ld, rows, op, C + O_PAD)
        torch.cuda.synchronize()
        assert not untouched or (o == SENTINEL).all(), "a refused call wrote the output"
        return rc

    assert call(hs=12, kv_hs=8) == -2  # MMT_ERR_UNSUPPORTED
    for kw in (dict(m=T - p + 1, rows=T - p + 1), dict(m=0, rows=0), dict(m=-1, rows=-1), dict(ns=0), dict(ns=9),
               dict(kv_ld=3 * C + 4), dict(q_ld=3 * C + 4), dict(kv_hs=hs + 4), dict(t_ld=3 * C + 4), dict(B=0),
               dict(H=0), dict(S=0), dict(S=-2), dict(p=0), dict(p=T), dict(rows=0), dict(rows=1), dict(rows=m + 1),
               dict(qp=null), dict(op=null), dict(k=None), dict(tk=None), dict(tv=None)):
        assert call(**kw) == -1, kw  # MMT_ERR_INVALID
    assert call(untouched=False) == 0  # and the same arguments unmodified run
    assert (o[:, C:] == SENTINEL).all() and torch.isfinite(o[:, :C].float()).all()
