"""CPU reference, error bound, fp32 emulation and input builders for the sample fan-out decode attention kernel
(attn_decode_fanout_kernel, csrc/mmt_decode_fanout.hip; mmt_op_attention_decode_fanout in include/mmt.h). Test
infrastructure only, torch on the CPU. The fp64 reference and the base bound are decode_ref's.

Canonical tensors (the GPU tests pack them into the engine's layouts): q bf16 [B, S, H, hs], sample s of prompt b;
per stream j the prompt's cache ks[j], vs[j] bf16 [B, H, T, hs], of which rows 0..n0-1 (the prefix) are read, and
the samples' tails tks[j], tvs[j] bf16 [B, S, H, cap, hs], of which rows 0..t-n0 are read (positions n0..t). Row
(b, s) attends over n = t + 1 keys: the prefix of prompt b, then its own tail.

The bound. The kernel walks the keys in tiles of KT = 64: ceil(n0 / 64) prefix tiles, then ceil((n - n0) / 64) tail
tiles, nt in all. Within a tile it does what attn_decode_kernel does over its whole window (fp32 scores, exp against
a maximum, fp32 sums of p and of p v), so decode_ref.tol covers the n-term sums, the scores, the exps and the
division. What the running state adds, per tile, read off merge_tile() in the kernel:

    alpha = exp(m_old - m_new);  l = l * alpha + sum_tile;  acc = acc * alpha

  2 x 2^-24 A   the two products l * alpha and acc * alpha: one fp32 rounding each, relative to the running sum
                (at most the final sum of magnitudes, A after the division).
  4 x 2^-24 A   alpha itself. The same fp32 number multiplies l and acc, so it cancels between numerator and
                denominator for the keys already merged; it only re-weights them against the keys still to come.
                A key whose exponent ends up x below the final maximum carries weight e^-x, and its chain of
                subtractions (s - m_tile, then m_i - m_i+1, ...) sums to x with one rounding of at most 2^-24 of
                each difference, so its weight is off by at most ~ x e^-x 2^-24 <= 2^-24 / e relative to the
                largest weight, per link; the hardware exp adds a couple of ulp per link. 4 x 2^-24 bounds both.

  6 x 2^-24 A per tile, and the factor 2 decode_ref.tol applies to its fp32 terms (the tolerance is evaluated at
  ref): 12 nt 2^-24 A = 3 nt 2^-22 A.

    tol_fan = decode_ref.tol(ref, A, n) + 3 nt 2^-22 A,   nt = ceil(n0 / 64) + ceil((n - n0) / 64)
"""
import math

import torch

import decode_ref as R

G = 16   # samples per workgroup (MMT_FANOUT_G)
KT = 64  # keys per tile (FAN_KT)
F64 = torch.float64


def tiles(n0, n):
    return -(-n0 // KT) + -(-(n - n0) // KT)


def tol_fan(ref, A, n, n0):
    return R.tol(ref, A, n) + 3 * tiles(n0, n) * 2.0 ** -22 * A


def worst_ratio(out, ref, A, n, n0):
    """decode_ref.worst_ratio against tol_fan. out, ref, A: [..., hs] of one shape. Returns (ratio, index)."""
    o = out.detach().cpu().to(F64)
    d = (o - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / tol_fan(ref, A, n, n0))
    r = torch.where(torch.isfinite(o), r, torch.full_like(r, math.inf))
    i = int(torch.argmax(r))
    return float(r.flatten()[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), r.shape))


def ratio_per_row_head(out, ref, A, n, n0):
    """[B, S, H]: the worst ratio of each (row, head)."""
    o = out.detach().cpu().to(F64)
    d = (o - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / tol_fan(ref, A, n, n0))
    r = torch.where(torch.isfinite(o), r, torch.full_like(r, math.inf))
    return r.max(dim=-1).values


def window(kp, kt, n0, L):
    """[B*S, H, n0 + L, hs]: every row's keys (or values) in window order, the prompt's prefix then its tail."""
    B, S = kt.shape[:2]
    pre = kp[:, None, :, :n0].expand(B, S, -1, -1, -1)
    return torch.cat((pre, kt[:, :, :, :L]), dim=3).reshape(B * S, kp.shape[1], n0 + L, kp.shape[-1])


def fanout_attention_ref(q, ks, vs, tks, tvs, n0, t, scale):
    """fp64 (decode_ref.decode_attention_ref over each row's assembled window). Returns (ref, A) [B, S, H, hs]."""
    B, S, H, hs = q.shape
    L = t - n0 + 1
    kw = [window(k, tk, n0, L) for k, tk in zip(ks, tks)]
    vw = [window(v, tv, n0, L) for v, tv in zip(vs, tvs)]
    ref, A = R.decode_attention_ref(q.reshape(B * S, H, hs), kw, vw, t, scale)
    return ref.view(B, S, H, hs), A.view(B, S, H, hs)


# ------------------------------------------------------------------------------------ fp32 emulation
BUGS = ("prefix_prompt", "tail_sample", "tail_long", "tail_short", "no_rescale", "early_tail")


def emulate_kernel(q, ks, vs, tks, tvs, n0, t, scale, bug=None):
    """attn_decode_fanout_kernel in fp32 torch ops, in its order of operations: the query times scale; per tile of
    64 keys the scores as one sequential sum over the head dims, the tile maximum, alpha = exp(m_old - m_new), the
    probabilities, their sum as ((p[kl] + p[kl + 16]) + p[kl + 32]) + p[kl + 48] per lane and an xor butterfly over
    the 16 lanes, l = l alpha + sum, acc = acc alpha, then acc += p v key by key; prefix tiles first, tail tiles
    after; acc / l, the streams added up, one bf16 rounding. Returns bf16 [B, S, H, hs].

    `bug` plants what the tests must be able to see: prefix_prompt reads the prefix of prompt b - 1, tail_sample
    the tail of sample s - 1, tail_long / tail_short a tail of one row more / less, no_rescale leaves l and acc
    unscaled when the maximum moves, early_tail merges the tail into the state from before the last prefix tile
    (that tile's update is lost)."""
    assert bug is None or bug in BUGS
    f32 = torch.float32
    B, S, H, hs = q.shape
    L = t - n0 + 1 + (1 if bug == "tail_long" else -1 if bug == "tail_short" else 0)
    qf = q.to(f32) * torch.tensor(scale, dtype=f32)
    lane = torch.arange(16)
    o = torch.zeros(B, S, H, hs, dtype=f32)
    for kp, vp, tk, tv in zip(ks, vs, tks, tvs):
        if bug == "prefix_prompt":
            kp, vp = kp.roll(1, 0), vp.roll(1, 0)
        if bug == "tail_sample":
            tk, tv = tk.roll(1, 1), tv.roll(1, 1)
        plan = [("p", k0, min(KT, n0 - k0)) for k0 in range(0, n0, KT)]
        plan += [("t", k0, min(KT, L - k0)) for k0 in range(0, L, KT)]
        m = torch.full((B, S, H), -math.inf, dtype=f32)
        l = torch.zeros(B, S, H, dtype=f32)
        acc = torch.zeros(B, S, H, hs, dtype=f32)
        last_prefix = -(-n0 // KT) - 1
        for ti, (kind, k0, kt) in enumerate(plan):
            if kind == "p":
                K = kp[:, None, :, k0:k0 + kt].to(f32).expand(B, S, H, kt, hs)
                V = vp[:, None, :, k0:k0 + kt].to(f32).expand(B, S, H, kt, hs)
            else:
                K, V = tk[:, :, :, k0:k0 + kt].to(f32), tv[:, :, :, k0:k0 + kt].to(f32)
            if bug == "early_tail" and ti == last_prefix:
                saved = (m.clone(), l.clone(), acc.clone())
            a = torch.zeros(B, S, H, kt, dtype=f32)
            for i in range(hs):
                a = a + qf[..., None, i] * K[..., i]
            sc = torch.full((B, S, H, KT), -math.inf, dtype=f32)
            sc[..., :kt] = a
            mn = torch.maximum(m, sc.max(dim=-1).values)
            alpha = torch.ones_like(m) if bug == "no_rescale" else torch.exp(m - mn)
            p = torch.exp(sc - mn[..., None])
            p4 = p.view(B, S, H, 4, 16)
            w = ((p4[..., 0, :] + p4[..., 1, :]) + p4[..., 2, :]) + p4[..., 3, :]
            for off in (8, 4, 2, 1):
                w = w + w[..., lane ^ off]
            l = l * alpha + w[..., 0]
            acc = acc * alpha[..., None]
            m = mn
            for key in range(kt):
                acc = acc + p[..., key, None] * V[..., key, :]
            if bug == "early_tail" and ti == last_prefix:
                m, l, acc = saved
        o = o + acc / l[..., None]
    return o.to(torch.bfloat16)


# ------------------------------------------------------------------------------------ input builders
def _bf(x):
    return x.to(torch.bfloat16)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def build_random(B, S, H, T, hs, ns, cap, seed=0):
    """Everything ~ N(0, 1) rounded to bf16, every sample with its own query."""
    g = _gen(seed)
    q = _bf(torch.randn(B, S, H, hs, generator=g))
    ks = [_bf(torch.randn(B, H, T, hs, generator=g)) for _ in range(ns)]
    vs = [_bf(torch.randn(B, H, T, hs, generator=g)) for _ in range(ns)]
    tks = [_bf(torch.randn(B, S, H, cap, hs, generator=g)) for _ in range(ns)]
    tvs = [_bf(torch.randn(B, S, H, cap, hs, generator=g)) for _ in range(ns)]
    return q, ks, vs, tks, tvs


def _paired_q(B, S, H, hs, g):
    """q[b, s] = +q_b for even s, -q_b for odd s: a prefix key aligned with q_b scores high for the even samples
    of the prompt and low for the odd ones, which lets one shared prefix serve both halves of a test."""
    qb = _bf(torch.randn(B, H, hs, generator=g))
    sign = torch.where(torch.arange(S) % 2 == 0, 1.0, -1.0).to(torch.bfloat16)
    return qb, qb[:, None] * sign[None, :, None, None]


def prefix_candidates(n0):
    """first and last prefix row, either side of the first tile boundary, a low row"""
    return sorted({min(max(c, 0), n0 - 1) for c in (0, n0 - 1, KT - 1, KT, 3)})


def tail_candidates(L):
    return sorted({min(max(c, 0), L - 1) for c in (0, L - 1, KT - 1, KT, 1)})


def needle_value(hs):
    return R.needle_value(hs)


def build_needle(B, S, H, T, hs, ns, cap, n0, t, scale, seed=0, score=12.0):
    """decode_ref.build_needle's rules for the fan-out: one needle per (row, head, stream), a key of scaled score
    `score` against N(0, 1) for the rest whose value is 8 + (d mod 7) + an offset. Queries are paired (_paired_q).
    Even samples have their needle in the PREFIX: row pp[b, h, j] of prompt b's cache, key aligned with q_b, value
    offset b (prefix needles differ per prompt; the odd samples score it -score). Odd samples have theirs in the
    TAIL: row tp[b, s, h, j] of their own tail, key aligned with -q_b, value offset s (tail needles differ per
    sample). The candidates cover the first and last prefix row, tail row 0 and tail row t - n0. The stale rows a
    too-long window would meet hold the row's own needle key with the value negated: tail row t - n0 + 1 of every
    sample (when cap has one). Returns q, ks, vs, tks, tvs, pp [B, H, ns], tp [B, S, H, ns] (-1 for even samples)."""
    g = _gen(seed)
    L = t - n0 + 1
    qb, q = _paired_q(B, S, H, hs, g)
    ks = [_bf(torch.randn(B, H, T, hs, generator=g)) for _ in range(ns)]
    vs = [_bf(torch.randn(B, H, T, hs, generator=g)) for _ in range(ns)]
    tks = [_bf(torch.randn(B, S, H, cap, hs, generator=g)) for _ in range(ns)]
    tvs = [_bf(torch.randn(B, S, H, cap, hs, generator=g)) for _ in range(ns)]
    qd = qb.to(F64)
    key = _bf(qd * score / (scale * (qd * qd).sum(-1, keepdim=True)))  # [B, H, hs], aligned with q_b
    val = needle_value(hs)
    pc, tc = torch.tensor(prefix_candidates(n0)), torch.tensor(tail_candidates(L))
    pp = pc[torch.arange(B * H * ns).view(B, H, ns) % len(pc)]
    tp = tc[torch.arange(B * S * H * ns).view(B, S, H, ns) % len(tc)]
    tp[:, 0::2] = -1
    for j in range(ns):
        for b in range(B):
            for h in range(H):
                ks[j][b, h, pp[b, h, j]] = key[b, h]
                vs[j][b, h, pp[b, h, j]] = _bf(val + b)
                for s in range(S):
                    own = key[b, h] if s % 2 == 0 else -key[b, h]
                    if s % 2 == 1:
                        tks[j][b, s, h, tp[b, s, h, j]] = own
                        tvs[j][b, s, h, tp[b, s, h, j]] = _bf(val + s)
                    if L < cap:
                        tks[j][b, s, h, L] = own
                        tvs[j][b, s, h, L] = _bf(-(val + s))
    return q, ks, vs, tks, tvs, pp, tp


def build_flat(B, S, H, T, hs, ns, cap, seed=0):
    """q = 0, integer values in [-8, 8], random keys: with n a power of two every probability is exactly 1, every
    alpha too, both sums are exact and the division is by a power of two, so the output is bf16(mean) bit for bit."""
    g = _gen(seed)
    q = torch.zeros(B, S, H, hs, dtype=torch.bfloat16)
    ks = [_bf(torch.randn(B, H, T, hs, generator=g)) for _ in range(ns)]
    tks = [_bf(torch.randn(B, S, H, cap, hs, generator=g)) for _ in range(ns)]
    vs = [_bf(torch.randint(-8, 9, (B, H, T, hs), generator=g).to(torch.float32)) for _ in range(ns)]
    tvs = [_bf(torch.randint(-8, 9, (B, S, H, cap, hs), generator=g).to(torch.float32)) for _ in range(ns)]
    return q, ks, vs, tks, tvs


def flat_expected(vs, tvs, n0, t):
    """bf16 [B, S, H, hs]: the sum over the streams of the mean of each row's window, exact, rounded once."""
    n = t + 1
    assert n & (n - 1) == 0, "the flat case is exact only for a power-of-two window"
    B, S = tvs[0].shape[:2]
    m = sum(window(v, tv, n0, n - n0).to(F64).sum(dim=2) / n for v, tv in zip(vs, tvs))
    assert torch.equal(m.to(torch.float32).to(F64), m)
    return m.to(torch.float32).to(torch.bfloat16).view(B, S, *m.shape[1:])


def build_shifted(B, S, H, T, hs, ns, cap, scale, seed=0, shift=100.0):
    """Paired queries; every prefix key carries +shift along q_b and every tail key -shift along q_b. Even samples
    (q = q_b) then score the whole prefix near +shift and their tail near -shift: the running maximum is set by
    the first tile and the tail underflows against it. Odd samples (q = -q_b) see the prefix near -shift and
    their tail near +shift: the first tail tile rescales everything merged so far to nothing."""
    g = _gen(seed)
    qb, q = _paired_q(B, S, H, hs, g)
    qd = qb.to(F64)
    add = qd * shift / (scale * (qd * qd).sum(-1, keepdim=True))  # [B, H, hs]
    ks = [_bf(torch.randn(B, H, T, hs, generator=g).to(F64) + add[:, :, None]) for _ in range(ns)]
    vs = [_bf(torch.randn(B, H, T, hs, generator=g)) for _ in range(ns)]
    tks = [_bf(torch.randn(B, S, H, cap, hs, generator=g).to(F64) - add[:, None, :, None]) for _ in range(ns)]
    tvs = [_bf(torch.randn(B, S, H, cap, hs, generator=g)) for _ in range(ns)]
    return q, ks, vs, tks, tvs
