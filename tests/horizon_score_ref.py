"""CPU restatement of the scoring rules (include/mmt.h: mmt_horizon_score), in fp64 numpy, on top of horizon_ref (rule 1,
the order of rule 4) and forecast_ref.path_weights (rule 2). Test infrastructure only.

realised(tok, values, is_percent, origin)  rule 1 on the realised rows [B, N]: horizon_ref.paths.
records(x, a, dead, real, stats, qval, hit, levels, barriers)
    rules 2 - 7 for one prompt. x fp64 [S, N] and dead [S] from horizon_ref.paths, a fp64 [S] log-weights or None,
    real = (x*, hi*, lo*, d*, dead*) of the prompt's realised row ([N] each), stats [N, 12] / qval [N, nq] / hit [N,
    nb] the forecast to score (the device's own in the GPU tests, so that sc[3..5], pin and bs compare bit for bit).
    Returns a dict: sc [N, 8], pin [N, nq], bs [N, nb], crps_bound, pit_bound [N].
tables(sc, pin, bs, stats, qval, hit, dstar, barriers, bins)
    rule 8 from records [B, N, .]: plain Python loops, every cell a serial sum from 0.0 over b ascending, so a device
    that follows the rule gives these bits.
energy(x, w, xr)   the CRPS in its energy form, sum w |x - x*| / W - 1/2 sum sum w w' |x - x'| / W^2, by brute force
    in Python floats (math.fsum): what the integral form of rule 3 is checked against.

The bounds, derived from the rule and the number formats, not from any kernel's error (RTOL and EPS as in horizon_ref).
  Without weights every w is 1, the prefix P_m is the integer m and F_m = m / n is one division of exact operands: the
  same bits anywhere. Every term of rule 3 is non-negative, so the sum in another order moves by at most (S + 16) 2^-53
  of itself: CRPS within RTOL = 1e-12 relative. The PIT's masses are integers (or halves): exact.
  With weights every w carries a relative error up to EPS = 4 * 2^-24 (a device expf against numpy's). Write e_s for
  it, |e_s| <= EPS. A ratio R = sum w f / W with 0 <= f <= 1 becomes sum w (1 + e) f / sum w (1 + e), and R' - R =
  sum w e (f - R) / (W (1 + e-bar)), so |R' - R| <= EPS' sum w |f - R| / W with EPS' = EPS / (1 - EPS). For 0 <= f <= 1
  sum w |f - R| / W <= sum w f / W + R = 2 R, and by the same argument on 1 - f it is <= 2 (1 - R).
    PIT: f = [x < x*] + 0.5 [x == x*], so it moves by <= 2 EPS' min(p, 1 - p), plus RTOL p for the two sums in another
    order.
    CRPS: F_m is such a ratio with f = [place <= m], where sum w |f - F| / W = 2 F (1 - F) exactly: dF <= 2 EPS' F (1 -
    F) <= 2 EPS' min(F, 1 - F). A gap's term t(F) = (s - a) F^2 + (b - s) (1 - F)^2 then moves by at most
    2 dF ((s - a) F + (b - s) (1 - F)) + dF^2 (b - a) <= 4 EPS' ((s - a) F^2 + (b - s) (1 - F)^2) + 4 EPS'^2 (b - a)
    = 4 EPS' t + 4 EPS'^2 (b - a). Summed over the gaps: 4 EPS' (the gap sum) + 4 EPS'^2 (x_(n) - x_(1)): the weights
    move the CRPS by a relative 4 EPS', tighter than 4 EPS times the range. The fp64 prefix in another order moves F by
    at most RTOL F <= RTOL absolutely, hence a term by <= 2 RTOL (b - a) and the sum by 2 RTOL (x_(n) - x_(1)); the sum
    of the non-negative terms itself by RTOL of itself. The tail is one subtraction of bit-exact operands: exact.
    Together: RTOL crps + (2 RTOL + 4 EPS'^2) range + 4 EPS' gap sum.
  x*, hi*, lo* come from rule 1, one IEEE operation per line: bit for bit, as x in horizon_ref.

The input family of the GPU tests (case): horizon_ref.case plus one realised row per prompt and problem, its kind
cycling over: a copy of one of the prompt's paths, an independent draw, a row below every path and a row above."""
import functools
import math

import numpy as np

import forecast_ref as F
import horizon_ref as H

RTOL = H.RTOL
EPS = H.EPS
EPS1 = EPS / (1.0 - EPS)
SAMPLES = [1, 2, 15, 16, 17, 255, 256, 257, 1000, 4096]
STEPS = [1, 2, 33]
KINDS = ("copy", "draw", "below", "above")


def realised(tok, values, is_percent, origin=None):
    return H.paths(tok, values, is_percent, origin)


def sgn(v):
    return 1 if v > 0 else -1 if v < 0 else 0


def records(x, a, dead, real, stats, qval, hit, levels, barriers):
    S, N = x.shape
    nq, nb = len(levels), len(barriers)
    xr, hr, lr, dr, rdead = real
    weighted = a is not None
    w, _, live = F.path_weights(np.zeros(S) if a is None else a, dead)
    out = {"sc": np.full((N, 8), np.nan), "pin": np.full((N, nq), np.nan), "bs": np.full((N, nb), np.nan),
           "crps_bound": np.zeros(N), "pit_bound": np.zeros(N), "live": live}
    if live == 0 or rdead:
        return out
    W = w.sum()
    keep = np.nonzero(w > 0)[0]
    wk = w[keep]
    for j in range(N):
        xj, xs_ = x[keep, j], float(xr[j])
        order = np.lexsort((keep, xj))  # (x, s) ascending
        xo = xj[order]
        P = np.cumsum(wk[order])
        lo_x, hi_x = xo[:-1], xo[1:]
        s = np.minimum(hi_x, np.maximum(lo_x, xs_))
        Fm = P[:-1] / W
        terms = (s - lo_x) * (Fm * Fm) + (hi_x - s) * ((1.0 - Fm) * (1.0 - Fm))
        gaps = float(terms.sum())
        tail = xo[0] - xs_ if xs_ < xo[0] else xs_ - xo[-1] if xs_ > xo[-1] else 0.0
        crps = gaps + tail
        pit = (wk[xj < xs_].sum() + 0.5 * wk[xj == xs_].sum()) / W
        st = stats[j]
        sc = out["sc"][j]
        sc[0], sc[1], sc[2] = xs_, crps, pit
        sc[3] = st[0] - xs_
        sc[4] = st[3 + sgn(xs_)]
        sc[5] = st[6 + int(dr[j])]
        sc[6], sc[7] = hr[j], lr[j]
        for k, lv in enumerate(levels):
            q = qval[j, k]
            out["pin"][j, k] = (xs_ - q) * (lv - (1.0 if xs_ < q else 0.0))
        for k, u in enumerate(barriers):
            o = 1.0 if (hr[j] >= u if u > 0 else lr[j] <= u) else 0.0
            e = hit[j, k] - o
            out["bs"][j, k] = e * e
        if weighted:
            rng = float(xo[-1] - xo[0])
            out["crps_bound"][j] = RTOL * crps + (2 * RTOL + 4 * EPS1 * EPS1) * rng + 4 * EPS1 * gaps
            out["pit_bound"][j] = 2 * EPS1 * min(pit, 1.0 - pit) + RTOL * pit
        else:
            out["crps_bound"][j] = RTOL * crps
    return out


def argmax3(m):
    k = 0
    if m[1] > m[k]:
        k = 1
    if m[2] > m[k]:
        k = 2
    return k


def tables(sc, pin, bs, stats, qval, hit, dstar, barriers, bins):
    """sc [B, N, 8], pin / qval [B, N, nq], bs / hit [B, N, nb], stats [B, N, 12], dstar int [B, N]."""
    B, N = sc.shape[:2]
    nq, nb = pin.shape[2], bs.shape[2]
    agg, aggq, aggb, pit = np.zeros((N, 10)), np.zeros((N, nq, 2)), np.zeros((N, nb, 3)), np.zeros((N, bins))
    for j in range(N):
        for b in range(B):
            r, st = [float(v) for v in sc[b, j]], [float(v) for v in stats[b, j]]
            if r[0] != r[0]:
                continue
            add = [1.0, r[1], abs(r[0]), abs(r[3]), r[3] * r[3], r[4],
                   1.0 if argmax3(st[2:5]) == 1 + sgn(r[0]) else 0.0, r[5],
                   1.0 if argmax3(st[5:8]) == 1 + int(dstar[b, j]) else 0.0, st[1]]
            for k in range(10):
                agg[j, k] = float(agg[j, k]) + add[k]
            for k in range(nq):
                aggq[j, k, 0] = float(aggq[j, k, 0]) + float(pin[b, j, k])
                aggq[j, k, 1] = float(aggq[j, k, 1]) + (1.0 if r[0] <= float(qval[b, j, k]) else 0.0)
            for k, u in enumerate(barriers):
                o = 1.0 if (r[6] >= u if u > 0 else r[7] <= u) else 0.0
                aggb[j, k, 0] = float(aggb[j, k, 0]) + float(bs[b, j, k])
                aggb[j, k, 1] = float(aggb[j, k, 1]) + float(hit[b, j, k])
                aggb[j, k, 2] = float(aggb[j, k, 2]) + o
            pit[j, min(bins - 1, int(math.floor(r[2] * float(bins))))] += 1.0
    return agg, aggq, aggb, pit


def energy(x, w, xr):
    """The energy form of the CRPS of the weighted sample (x, w) at xr, Python floats."""
    x, w = [float(v) for v in x], [float(v) for v in w]
    W = math.fsum(w)
    first = math.fsum(wi * abs(xi - xr) for xi, wi in zip(x, w)) / W
    second = math.fsum(wi * wj * abs(xi - xj) for xi, wi in zip(x, w) for xj, wj in zip(x, w)) / (W * W)
    return first - 0.5 * second


def kind_of(S, N, V, p, b):
    return KINDS[(b + p + SAMPLES.index(S) + STEPS.index(N) + H.VS.index(V)) % 4] if (
        S in SAMPLES and N in STEPS and V in H.VS) else KINDS[(b + p) % 4]


@functools.lru_cache(maxsize=None)
def case(S, N, V, sigma, seed=0, levels=H.LEVELS, barriers=H.BARRIERS):
    """horizon_ref.case plus the realised rows: real int64 [2][3, N], real_origin int64 [3] (the value problem's),
    kinds [2][3], and rz[p] = realised(...) of problem p."""
    c = dict(H.case(S, N, V, sigma, seed, levels, barriers))
    rng = np.random.default_rng(31337 * seed + 104729 * S + 17 * N + V)
    real = [np.zeros((H.PROMPTS, N), dtype=np.int64) for _ in range(2)]
    real_origin = np.zeros(H.PROMPTS, dtype=np.int64)
    kinds = [[kind_of(S, N, V, p, b) for b in range(H.PROMPTS)] for p in range(2)]
    for p in range(2):
        for b in range(H.PROMPTS):
            k = kinds[p][b]
            s = int(rng.integers(0, S))
            draw, o = rng.integers(0, V, size=N), int(rng.integers(0, V))
            if k == "copy":
                row, o = c["tok"][p][b * S + s], int(c["origin"][b * S + s])
            elif k == "draw":
                row = draw
            elif k == "below":  # the smallest change a row can show: the lowest value at every step, from the highest
                row, o = np.zeros(N, dtype=np.int64), V - 1
            else:
                row, o = np.full(N, V - 1, dtype=np.int64), 0
            real[p][b] = row
            if p == 1:
                real_origin[b] = o
    c.update(real=real, real_origin=real_origin, kinds=kinds,
             rz=[realised(real[p], c["values"], p == 0, real_origin) for p in range(2)])
    return c
