"""CPU restatement of mmt_resample's rule (include/mmt.h), in numpy: the fp32 weights as the kernel forms them, every
sum in fp64 (a serial cumulative sum; the kernel's tree differs from it by roundings the tests bound). Test
infrastructure only.

accumulate(logw, lps, j0, j1)       rule 1: a_s = logw + the columns of the given matrices, serial, NaN as -inf
resample_prompt(a, thr, seed, b, pos)  rules 1 - 4 for one prompt; returns a dict:
    ess, trigger, live        ESS = W^2 / Q, whether ESS < thr * S, whether any path is live
    evidence                  mx + log(W / S) (what a trigger adds to log_evidence; -inf without a live path)
    ancestor [S]              local row per slot (the identity without a trigger)
    neighbor [S]              the live row across the nearest prefix boundary (the ancestor itself when there is none)
    margin [S]                distance of (s + u) / S * W to that boundary, relative to W (inf when there is none)
    e [S], W                  the weights and their sum
"""
import math

import numpy as np

from sampling_ref import M32, mmt_hash

SALT = 0x52534D50


def uniform(seed, b, pos):
    seed &= 2 ** 64 - 1
    key = mmt_hash(seed & M32, seed >> 32, SALT)
    h = mmt_hash(key, b & M32, pos & M32)
    return ((h >> 8) + 0.5) * 2.0 ** -24


def accumulate(logw, lps, j0, j1):
    """Rule 1's sum for every row: logw fp64 [R], lps a list of fp32 [R, N] (ascending modality). fp64 [R]."""
    a = np.array(logw, dtype=np.float64)
    a[np.isnan(a)] = -np.inf
    with np.errstate(all="ignore"):
        for j in range(j0, j1):
            for lp in lps:
                t = np.asarray(lp)[:, j].astype(np.float64)
                t[np.isnan(t)] = -np.inf
                a = a + t
    a[np.isnan(a)] = -np.inf
    return a


def weights(a):
    """Rule 2's fp32 weights of one prompt, as fp64 values, and mx."""
    mx = a.max()
    with np.errstate(all="ignore"):
        d = (a - mx).astype(np.float32)
        e = np.where(d == 0, np.float32(1.0), np.exp(d, dtype=np.float32)).astype(np.float32)
    return e.astype(np.float64), mx


def resample_prompt(a, ess_threshold, seed, b, pos):
    a = np.asarray(a, dtype=np.float64)
    S = len(a)
    ident = np.arange(S)
    out = {"ancestor": ident.copy(), "neighbor": ident.copy(), "margin": np.full(S, math.inf), "trigger": False,
           "live": True, "ess": math.nan, "evidence": -math.inf, "e": np.zeros(S), "W": 0.0}
    if a.max() == -np.inf:
        out["live"] = False
        return out
    e, mx = weights(a)
    W, Q = e.sum(), (e * e).sum()
    out.update(e=e, W=W, ess=W * W / Q, evidence=mx + math.log(W / S))
    out["trigger"] = bool(out["ess"] < ess_threshold * S)
    if not out["trigger"]:
        return out
    u = uniform(seed, b, pos)
    live = np.nonzero(e > 0)[0]
    kp = np.cumsum(e)[live]  # inclusive prefix at the live rows
    n = len(live)
    target = (np.arange(S, dtype=np.float64) + u) / S * W
    j = np.minimum(np.searchsorted(kp, target, side="left"), n - 1)
    out["ancestor"] = live[j]
    out["neighbor"] = live[j].copy()
    if n > 1:
        below = np.where(j > 0, target - kp[np.maximum(j - 1, 0)], math.inf)  # towards the previous live row
        above = np.where(j < n - 1, kp[j] - target, math.inf)  # towards the next one
        down = below <= above
        out["margin"] = np.where(down, below, above) / W
        out["neighbor"] = np.where(down, live[np.maximum(j - 1, 0)], live[np.minimum(j + 1, n - 1)])
    return out


def check_ancestors(ref, anc, delta):
    """The clear / ambiguous rule on local rows: (ambiguous slots, failing slots)."""
    anc = np.asarray(anc)
    clear = ref["margin"] >= delta
    ok = (anc == ref["ancestor"]) | (~clear & (anc == ref["neighbor"]))
    return int((~clear).sum()), [int(s) for s in np.nonzero(~ok)[0]]


def family(S, sigma, seed, prompts=3):
    """The GPU tests' inputs: `prompts` rows of S log-weights N(0, sigma^2), fp64 [prompts, S]. The prompts differ
    (independent draws; prompt 1 shifted by -50, which the rule must not notice)."""
    rng = np.random.default_rng(100003 * seed + 17 * S + int(10 * sigma))
    a = rng.normal(0.0, 1.0, size=(prompts, S)) * sigma
    if prompts > 1:
        a[1] -= 50.0
    return a


SIGMAS = [0.0, 0.3, 2.0, 8.0]
SAMPLES = [1, 2, 15, 16, 17, 64, 257, 1000, 4096]
SEEDS = list(range(8))
THRESHOLDS = [0.6, 2.0]  # the ESS / S thresholds the GPU tests resample with (0 and negative never trigger)
POS = 5  # and the position they key the draw with
