"""CPU restatement of the sampling rule of mmt_sample (include/mmt.h), in numpy: fp64 after the one fp32 multiply
of step 1. Test infrastructure only.

sample_row / sample_rows return, per row: the token, its log-probability, and what a comparison with an fp32
device result needs to know about how close the row is to a decision boundary:
  margin_u   distance of u * S to the nearest prefix boundary between two kept tokens, divided by S (inf when the
             kept set has one token)
  margin_p   distance of top_p * S to the nearest group mass of step 4, divided by S (inf when top-p is off or
             top_p <= 0)
  neighbor   the kept token on the other side of that nearest prefix boundary (the token itself when there is none)
"""
import math

import numpy as np

M32 = 0xFFFFFFFF
SALT = 0x53414D50


def mmt_hash(a, b, c):
    """csrc/mmt_common.h mmt_hash, on Python ints."""
    h = ((a * 0x9E3779B1) & M32) ^ (((b + 0x7F4A7C15) & M32) * 0x85EBCA77 & M32) ^ (((c + 0x165667B1) & M32) * 0xC2B2AE3D & M32)
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    h ^= h >> 16
    return h


def seed_key(seed):
    seed &= 2 ** 64 - 1
    return mmt_hash(seed & M32, seed >> 32, SALT)


def uniform(seed, row, pos):
    """Step 5: u in (0, 1), exact in fp64."""
    h = mmt_hash(seed_key(seed), row & M32, pos & M32)
    return ((h >> 8) + 0.5) * 2.0 ** -24


def scaled(logits, temperature):
    """Step 1: one fp32 multiply by the fp32 reciprocal of the temperature; NaN as -inf. fp32 in, fp32 out."""
    l = np.asarray(logits, dtype=np.float32)
    with np.errstate(all="ignore"):
        z = l * (np.float32(1.0) / np.float32(temperature)) if temperature != 0 else l.copy()
    z = z.astype(np.float32)
    z[np.isnan(z)] = -np.inf
    return z


def _weights(zd, m, kept):
    with np.errstate(all="ignore"):
        e = np.where(zd == m, 1.0, np.exp(zd - m))
    e[np.isnan(e)] = 0.0
    return np.where(kept, e, 0.0)


def sample_row(logits, temperature, top_k, top_p, seed, row, pos):
    """One row. Returns a dict: token, logprob, margin_u, margin_p, neighbor, kept (bool [V]), u."""
    V = len(logits)
    u = uniform(seed, row, pos)
    out = {"u": u, "margin_u": math.inf, "margin_p": math.inf}
    z = scaled(logits, temperature)
    zd = z.astype(np.float64)
    m = zd.max()
    if m == -np.inf:
        out.update(token=0, logprob=math.nan, neighbor=0, kept=np.zeros(V, bool))
        return out
    if temperature == 0:
        e = _weights(zd, m, np.ones(V, bool))
        t = int(np.argmax(zd == m))
        out.update(token=t, logprob=-math.log(e.sum()), neighbor=t, kept=zd == m)
        return out
    kept = np.ones(V, bool)
    if 0 < top_k < V:
        t_k = np.sort(zd)[::-1][top_k - 1]
        kept = zd >= t_k
    e = _weights(zd, m, kept)
    S = e.sum()
    p = float(np.float32(top_p))
    if p < 1.0:
        vals = np.unique(zd[kept])[::-1]  # distinct kept values, descending
        if p <= 0.0:
            t_p = vals[0]
        else:
            order = np.argsort(-zd, kind="stable")
            cum = np.cumsum(e[order])
            zs = zd[order]
            # mass of { z >= v }: the cumulative sum at the last sorted position holding v
            lastpos = np.searchsorted(-zs, -vals, side="right") - 1
            masses = cum[lastpos]
            reach = np.nonzero(masses >= p * S)[0]
            gi = int(reach[0]) if len(reach) else len(vals) - 1
            t_p = vals[gi]
            out["margin_p"] = float(np.min(np.abs(masses - p * S)) / S)
        kept = kept & (zd >= t_p)
        e = _weights(zd, m, kept)
        S = e.sum()
    prefix = np.cumsum(e)
    target = u * S
    ki = np.nonzero(kept & (e > 0))[0]  # kept tokens, vocabulary order
    kp = prefix[ki]
    j = int(np.searchsorted(kp, target, side="left"))
    j = min(j, len(ki) - 1)
    t = int(ki[j])
    neighbor = t
    if len(ki) > 1:
        below = target - kp[j - 1] if j > 0 else math.inf  # boundary towards the previous kept token
        above = kp[j] - target if j < len(ki) - 1 else math.inf  # towards the next one
        if below <= above:
            out["margin_u"], neighbor = float(below / S), int(ki[j - 1])
        else:
            out["margin_u"], neighbor = float(above / S), int(ki[j + 1])
    out.update(token=t, logprob=float(math.log(e[t] / S)), neighbor=neighbor, kept=kept)
    return out


def sample_rows(logits, temperature, top_k, top_p, seed, pos, row0=0):
    """Rows b of an [B, V] array at (seed, row0 + b, pos). Returns a dict of arrays over the rows."""
    rows = [sample_row(logits[b], temperature, top_k, top_p, seed, row0 + b, pos) for b in range(len(logits))]
    return {
        "token": np.array([r["token"] for r in rows], dtype=np.int64),
        "logprob": np.array([r["logprob"] for r in rows], dtype=np.float64),
        "margin_u": np.array([r["margin_u"] for r in rows], dtype=np.float64),
        "margin_p": np.array([r["margin_p"] for r in rows], dtype=np.float64),
        "neighbor": np.array([r["neighbor"] for r in rows], dtype=np.int64),
        "kept": [r["kept"] for r in rows],
    }


def check_tokens(ref, tok, delta):
    """The clear / ambiguous rule: where both margins are at least delta the token must be the reference's, elsewhere
    the reference's or the stated neighbour. Returns (number of ambiguous rows, list of failing rows)."""
    tok = np.asarray(tok)
    clear = (ref["margin_u"] >= delta) & (ref["margin_p"] >= delta)
    ok = (tok == ref["token"]) | (~clear & (tok == ref["neighbor"]))
    return int((~clear).sum()), [int(b) for b in np.nonzero(~ok)[0]]
