"""CPU restatement of mmt_eval_positions (include/mmt.h), both stages, in fp64 numpy. Test infrastructure only.

records(logits, xb, yb, values, is_percent, t_begin)   stage 1: rec fp64 [B, T, 8]; rows before t_begin hold NaN
tables(rec, t_begin, bins)                             stage 2: (pos [T, 8], rel [3, bins, 3], pit [bins]), the
                                                       serial sums in the entry's order, so that applied to the
                                                       DEVICE's records it must reproduce the device's tables bit
                                                       for bit
mass_bound(m, V)                                       what a device mass (rec[1..4]) may differ by from `records`

The weights are restated as the rule states them: z - m is the fp32 subtraction (exact to reproduce), the exponential
of that fp32 number is taken in fp64. Masses are exact sums of those weights (math.fsum), divided once.

The bound of a mass. Write a mass as m = A / S with A the sum of the weights of a class (for the mid-PIT: of the tokens
below yb plus half the weight of yb, a sum of weights all the same) and S = A + B the sum of all of them.
  * The weights. A device weight is expf of the same fp32 argument, rounded to fp32; numpy's is exp in fp64. With
    eps = forecast_ref.EPS_W the relative difference of a weight (3 ulp of expf against 1 ulp, as the sampler tests take
    it), A' = A (1 + a) and B' = B (1 + b) with |a|, |b| <= eps, and
        A' / (A' + B') - A / (A + B) = A B (a - b) / ((A + B) (A' + B')) ,
    to first order m (1 - m) (a - b): at most 2 eps m (1 - m) <= 2 eps min(m, 1 - m). A class that holds every token
    with weight (m = 1) or none (m = 0) is exact: numerator and S are then the same sum, or the numerator is 0.
  * The sums. The device adds fp64 over the sampler's tree: thread t owns c = ceil(V / 256) | 1 consecutive elements
    (c additions), a 6-step shift scan over the lanes, the wave totals left to right (3): c + 9 roundings of 2^-53,
    each relative to a partial sum that is at most the total. The numerator's are relative to A <= m S, those of S to S;
    the PIT adds one more addition, every mass one division; fsum here adds one rounding and the division another. So a
    mass is off by at most m ((c + 9) + (c + 9) + 4) 2^-53. The bound taken is (c + 19) 2^-53 absolute, which covers
    this worst case for every m <= (c + 19) / (2 c + 22), i.e. every m <= 1 / 2; above one half the worst case is
    larger by up to (c + 3) 2^-53 (1e-14 at V = 8193), and what keeps the device inside the bound there is that the
    numerator and S run the same tree on leaves that differ only in the zeroed ones, so that most of their roundings
    are the same and cancel in the ratio. That is an observation about the summation, not a proof: should a row ever
    miss the bound by such an amount with m > 1 / 2, look here first. The first term, 2 eps min(m, 1 - m), dwarfs all
    of this unless m is within 1e-8 of 0 or 1.
"""
import math

import numpy as np

from forecast_ref import EPS_W

NAN = float("nan")


def weights(row):
    """The rule's weights of one row of fp32 logits: (e fp64 [V], z fp32 [V] with NaN as -inf, m). A row with no
    finite logit returns m = -inf and zero weights."""
    z = np.asarray(row, dtype=np.float32).copy()
    z[np.isnan(z)] = -np.inf
    m = z.max()
    if m == -np.inf:
        return np.zeros(len(z)), z, m
    with np.errstate(all="ignore"):
        d = (z - m).astype(np.float32)  # the fp32 subtraction
        e = np.where(z == m, 1.0, np.exp(d.astype(np.float64)))
    e[np.isnan(e)] = 0.0
    return e, z, m


def sign(v, origin_value, is_percent):
    """The reference's _get_direction_sign for numbers."""
    ch = v if is_percent else v - origin_value
    return 1 if ch > 0 else -1 if ch < 0 else 0


def record(row, x, y, values=None, is_percent=False):
    """One row's eight fields."""
    V = len(row)
    out = np.full(8, NAN)
    e, z, m = weights(row)
    if m == -np.inf or not (0 <= x < V and 0 <= y < V):
        return out
    S = math.fsum(e)
    out[0] = -np.inf if z[y] == -np.inf else (float(z[y]) - float(m)) - math.log(S)
    out[4] = (math.fsum(e[:y]) + 0.5 * e[y]) / S
    out[5] = float((z > z[y]).sum())
    if values is not None:
        v = np.asarray(values, dtype=np.float64)
        vo = 0.0 if is_percent else float(v[x])
        ch = v if is_percent else v - vo
        sg = (ch > 0).astype(np.int64) - (ch < 0).astype(np.int64)  # `sign`, over the vocabulary
        for k, s in ((1, -1), (2, 0), (3, 1)):
            out[k] = math.fsum(e[sg == s]) / S
        out[6] = float(sg[int(np.argmax(z == m))])  # the lowest index among the maxima
        out[7] = float(sg[y])
    return out


def records(logits, xb, yb, values=None, is_percent=False, t_begin=0):
    logits = np.asarray(logits, dtype=np.float32)
    B, T, V = logits.shape
    rec = np.full((B, T, 8), NAN)
    for b in range(B):
        for t in range(t_begin, T):
            rec[b, t] = record(logits[b, t], int(xb[b, t]), int(yb[b, t]), values, is_percent)
    return rec


def bin_of(p, bins):
    return min(bins - 1, int(math.floor(p * bins)))


def tables(rec, t_begin=0, bins=10):
    """Stage 2 on any records (the restatement's or the device's): every sum serial in fp64 from 0, a position's over
    b ascending, a reliability / PIT cell over t ascending of the positions' own sums."""
    rec = np.asarray(rec, dtype=np.float64)
    B, T, _ = rec.shape
    pos, rel, pit = np.zeros((T, 8)), np.zeros((3, bins, 3)), np.zeros(bins)
    with np.errstate(all="ignore"):
        for t in range(t_begin, T):
            prel, ppit = np.zeros((3, bins, 3)), np.zeros(bins)
            for b in range(B):
                r = rec[b, t]
                if np.isnan(r[5]):
                    continue
                has_dir = not np.isnan(r[6])
                pos[t, 0] += 1.0
                pos[t, 4] += -r[0]
                pos[t, 5] += 1.0 if r[5] == 0 else 0.0
                ppit[bin_of(r[4], bins)] += 1.0
                if not has_dir:
                    continue
                pos[t, 1] += 1.0 if r[6] == r[7] else 0.0
                pos[t, 2] += 1.0 if r[6] != r[7] else 0.0
                pos[t, 3] += r[1 + int(r[6]) + 1]
                pos[t, 6] += 1.0
                pos[t, 7] += r[1 + int(r[7]) + 1]
                for d in range(3):
                    k = bin_of(r[1 + d], bins)
                    prel[d, k, 0] += 1.0
                    prel[d, k, 1] += r[1 + d]
                    prel[d, k, 2] += 1.0 if r[7] == d - 1 else 0.0
            rel = rel + prel
            pit = pit + ppit
    return pos, rel, pit


def chunk(V):
    """The sampler's per-thread element count."""
    return ((V + 255) // 256) | 1


def mass_bound(m, V):
    m = np.asarray(m, dtype=np.float64)
    return 2 * EPS_W * np.minimum(m, 1 - m) + (chunk(V) + 19) * 2.0 ** -53


def series(V, kind, seed=0):
    """The vocabularies of the tests, fp64 [V] non-decreasing: "value" (distinct values of both signs), "percent" (the
    same, read as a percent series), "repeated" (runs of equal values and exact zeros)."""
    rng = np.random.default_rng(6000 + V + seed)
    v = np.sort(rng.normal(0.25, 2.0, size=V))
    if kind == "repeated":
        v = np.sort(np.round(v))
    return v


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)
