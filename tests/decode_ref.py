"""CPU reference, error bound, fp32 emulation and input builders for the KV-cache decode attention kernel
(attn_decode_kernel, csrc/mmt_decode.hip; mmt_op_attention_decode in include/mmt.h). Test infrastructure only,
torch on the CPU, no GPU needed.

Canonical tensors (the GPU tests pack them into the engine's cache layouts): q bf16 [B, H, hs]; per stream j
ks[j], vs[j] bf16 [B, H, T, hs], every row finite. The query of position t sees rows 0..t (n = t + 1 keys); what
the builders put into rows above t is the "stale" content a too-long window would read.

The bound. The kernel does fp32 scalar arithmetic on the bf16 values and rounds its output once, so per element
(b, h, d), with ref = sum_j softmax_j . v_j and A = sum_j softmax_j . |v_j| in exact arithmetic,

    |out - ref| <= tol = 2^-8 |ref| + (n + 256) 2^-22 A

  2^-8 |ref|      the single round-to-nearest-even bf16 rounding: half an ulp is at most 2^-8 of the value.
  n 2^-24 A       each of the two length-n fp32 sums (probabilities times values, and the probabilities): a sum of
                  n terms carries at most n roundings of 2^-24 relative to the sum of magnitudes, which is A for
                  the numerator and turns into a relative error of the quotient, again times A at most, for the
                  denominator.
  256 2^-24 A     the hs <= 64 term score (its error enters the exponent, so it is a relative error of a
                  probability: |score| 2^-24 per term, scores of a few tens at the most), the hardware exp
                  (a few ulp) and the division.
  the factor 2    (2^-22 where the three lines above give 2 (n + 256) 2^-24 = (n + 256) 2^-23): the tolerance
                  is evaluated at ref, not at the unrounded fp32 value the rounding term strictly refers to.
"""
import math

import torch

HEAD_SIZES = (8, 16, 24, 32, 48, 64)
F64 = torch.float64


def decode_attention_ref(q, ks, vs, t, scale):
    """fp64 on the bf16 values as given. Returns (ref, A), each fp64 [B, H, hs]: the sum over the streams of
    softmax(scale q.k_s, s <= t) . v, and the same with |v|."""
    n = t + 1
    qd = q.to(F64)
    ref = torch.zeros(qd.shape, dtype=F64)
    A = torch.zeros(qd.shape, dtype=F64)
    for k, v in zip(ks, vs):
        kd, vd = k[:, :, :n].to(F64), v[:, :, :n].to(F64)
        sc = scale * torch.einsum("bhd,bhsd->bhs", qd, kd)
        p = torch.softmax(sc, dim=-1)
        ref += torch.einsum("bhs,bhsd->bhd", p, vd)
        A += torch.einsum("bhs,bhsd->bhd", p, vd.abs())
    return ref, A


def tol(ref, A, n):
    return 2.0 ** -8 * ref.abs() + (n + 256) * 2.0 ** -22 * A


def worst_ratio(out, ref, A, n):
    """max over the elements of |out - ref| / tol (a NaN or an infinity counts as inf; 0 / 0 as 0).
    Returns (ratio, (b, h, d))."""
    o = out.detach().cpu().to(F64)
    d = (o - ref).abs()
    tl = tol(ref, A, n)
    r = torch.where(d == 0, torch.zeros_like(d), d / tl)
    r = torch.where(torch.isfinite(o), r, torch.full_like(r, math.inf))
    i = int(torch.argmax(r))
    return float(r.flatten()[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), r.shape))


# ------------------------------------------------------------------------------------ fp32 emulation
def emulate_kernel(q, ks, vs, t, scale, drop=None, extra=0, swap_v=False, no_max=False):
    """attn_decode_kernel in fp32 torch ops, in its order of operations: the query times scale, scores
    accumulated two terms at a time, block max, exp, the probability sum as 256 strided thread partials + a
    butterfly per 64 lanes + four wave sums, values as four strided groups, (g0 + g1 + g2 + g3) / sum, the
    streams added up, one bf16 rounding. Returns bf16 [B, H, hs].

    The keywords plant the bugs the tests must be able to see: drop (long [B, H, nstreams], -1 = none) removes
    that key of the window, extra = 1 reads one row past the window, swap_v pairs stream j's probabilities
    with the values of stream j + 1, no_max skips the max subtraction."""
    f32 = torch.float32
    B, H, hs = q.shape
    n = t + 1 + extra
    qf = q.to(f32) * torch.tensor(scale, dtype=f32)
    if swap_v:
        vs = list(vs[1:]) + list(vs[:1])
    o = torch.zeros(B, H, hs, dtype=f32)
    for j, (k, v) in enumerate(zip(ks, vs)):
        kf, vf = k[:, :, :n].to(f32), v[:, :, :n].to(f32)
        acc = torch.zeros(B, H, n, dtype=f32)
        for i in range(0, hs, 2):
            acc = acc + (qf[:, :, None, i] * kf[..., i] + qf[:, :, None, i + 1] * kf[..., i + 1])
        if drop is not None:
            s_idx = torch.arange(n)[None, None, :]
            acc = torch.where(s_idx == drop[:, :, j, None], torch.full_like(acc, -math.inf), acc)
        mx = torch.zeros(B, H, 1, dtype=f32) if no_max else acc.max(dim=-1, keepdim=True).values
        p = torch.exp(acc - mx)
        # probability sum: thread tid adds p[tid], p[tid + 256], ...; xor butterfly over 64 lanes; 4 waves in order
        trips = (n + 255) // 256
        pp = torch.zeros(B, H, trips * 256, dtype=f32)
        pp[..., :n] = p
        pp = pp.view(B, H, trips, 256)
        part = torch.zeros(B, H, 256, dtype=f32)
        for i in range(trips):
            part = part + pp[:, :, i]
        w = part.view(B, H, 4, 64)
        lane = torch.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            w = w + w[..., lane ^ off]
        total = ((w[:, :, 0, 0] + w[:, :, 1, 0]) + w[:, :, 2, 0]) + w[:, :, 3, 0]
        # values: group g adds p_s v_s over s = g, g + 4, ...
        n4 = (n + 3) // 4
        p4 = torch.zeros(B, H, n4 * 4, dtype=f32)
        p4[..., :n] = p
        v4 = torch.zeros(B, H, n4 * 4, hs, dtype=f32)
        v4[:, :, :n] = vf
        p4, v4 = p4.view(B, H, n4, 4), v4.view(B, H, n4, 4, hs)
        g = torch.zeros(B, H, 4, hs, dtype=f32)
        for i in range(n4):
            g = g + p4[:, :, i, :, None] * v4[:, :, i]
        num = ((g[:, :, 0] + g[:, :, 1]) + g[:, :, 2]) + g[:, :, 3]
        o = o + num / total[..., None]
    return o.to(torch.bfloat16)


# ------------------------------------------------------------------------------------ input builders
def _bf(x):
    return x.to(torch.bfloat16)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def build_random(B, H, T, hs, ns, seed=0):
    """q, k, v ~ N(0, 1), rounded to bf16 (all T rows)."""
    g = _gen(seed)
    q = _bf(torch.randn(B, H, hs, generator=g))
    ks = [_bf(torch.randn(B, H, T, hs, generator=g)) for _ in range(ns)]
    vs = [_bf(torch.randn(B, H, T, hs, generator=g)) for _ in range(ns)]
    return q, ks, vs


def needle_candidates(t):
    """The key rows a window or loop bug loses, gains or shifts first: both ends, the last row of the first 256-key
    trip and the first of the second, a low row, and the first row of the last group of four."""
    n = t + 1
    return [min(max(c, 0), t) for c in (0, t, t - 1, 255, 256, 3, n - 1 - (n - 1) % 4)]


def needle_positions(B, H, ns, t, rot=0):
    """s* per (b, h, stream), long [B, H, ns]: the candidates in turn, starting at candidate `rot`."""
    cand = needle_candidates(t)
    slot = torch.arange(B * H * ns).view(B, H, ns)
    return torch.tensor(cand)[(slot + rot) % len(cand)]


def needle_value(hs):
    return 8.0 + (torch.arange(hs) % 7).to(torch.float32)


def build_needle(B, H, T, hs, ns, t, scale, seed=0, rot=0, score=12.0):
    """Random inputs with, in every stream, one key row s* set to q * score / (scale |q|^2): its scaled score
    is `score` against N(0, 1) for the rest, and that row's value is 8 + (d mod 7). A dropped, duplicated or
    misattributed key then moves the output by about 8, not by 1 / n. Row t + 1 (when the cache has one) is the
    stale row a too-long window would meet at its worst: the needle's key again, with the value negated.
    Returns q, ks, vs, s* [B, H, ns]."""
    q, ks, vs = build_random(B, H, T, hs, ns, seed)
    pos = needle_positions(B, H, ns, t, rot)
    qd = q.to(F64)
    key = _bf(qd * score / (scale * (qd * qd).sum(-1, keepdim=True)))  # [B, H, hs]
    val = _bf(needle_value(hs))
    bi, hi = torch.meshgrid(torch.arange(B), torch.arange(H), indexing="ij")
    for j in range(ns):
        ks[j][bi, hi, pos[:, :, j]] = key
        vs[j][bi, hi, pos[:, :, j]] = val
        if t + 1 < T:
            ks[j][:, :, t + 1] = key
            vs[j][:, :, t + 1] = -val
    return q, ks, vs, pos


def build_flat(B, H, T, hs, ns, seed=0):
    """q = 0, v integer-valued in [-8, 8], k random. With n a power of two every probability is exactly 1, both
    sums are exact in fp32 and the division is by a power of two: the output must equal bf16(mean) bit for bit,
    and a window of n - 1 or n + 1 keys cannot."""
    g = _gen(seed)
    q = torch.zeros(B, H, hs, dtype=torch.bfloat16)
    ks = [_bf(torch.randn(B, H, T, hs, generator=g)) for _ in range(ns)]
    vs = [_bf(torch.randint(-8, 9, (B, H, T, hs), generator=g).to(torch.float32)) for _ in range(ns)]
    return q, ks, vs


def flat_expected(vs, t):
    """bf16 [B, H, hs]: the sum over the streams of the mean of rows 0..t, exact in fp64, rounded once."""
    n = t + 1
    assert n & (n - 1) == 0, "the flat case is exact only for a power-of-two window"
    m = sum(v[:, :, :n].to(F64).sum(dim=2) / n for v in vs)
    assert torch.equal(m.to(torch.float32).to(F64), m)  # exact in fp32, so one rounding to bf16 below
    return m.to(torch.float32).to(torch.bfloat16)


def build_shifted(B, H, T, hs, ns, scale, seed=0, shift=60.0):
    """Random inputs with every key of a (b, h) carrying an added multiple of q, so that all scaled scores sit
    near +shift for even b * H + h and near -shift for odd. fp32 exp overflows above 88.7 and underflows below
    -87.3: at the default 60 a kernel without max subtraction is off only through lost precision, at 100 it
    returns inf / inf or 0 / 0."""
    q, ks, vs = build_random(B, H, T, hs, ns, seed)
    qd = q.to(F64)
    sign = torch.where((torch.arange(B * H).view(B, H) % 2) == 0, 1.0, -1.0).to(F64)
    add = qd * (sign * shift)[..., None] / (scale * (qd * qd).sum(-1, keepdim=True))
    ks = [_bf(k.to(F64) + add[:, :, None, :]) for k in ks]
    return q, ks, vs
