"""CPU restatement of mmt_eval_temperatures (include/mmt.h), both stages, and of the fit on top of it
(mmt_eval.fit_temperature / derive_temperature), in fp64 numpy on eval_ref.weights / eval_ref.sign. Test
infrastructure only.

records(logits, xb, yb, values, is_percent, temperatures, t_begin)   stage 1: rec fp64 [B, T, K, 4]; rows before
                                                                     t_begin hold NaN. z is the fp32 product of the
                                                                     logit with the fp32 inv_t = 1 / tau
realised(xb, yb, values, is_percent)                                 the realised sign of every row, fp64 [B, T] (NaN
                                                                     without values or with a token outside)
tables(rec, t_begin, bins, realised)                                 stage 2: (sum [K, 2], rel [K, 3, bins, 3]), the
                                                                     serial sums in the entry's order. A record holds
                                                                     the log score and the three masses, not the sign
                                                                     of yb, so the realised signs come beside it
fit(temperatures, rows, nll_sum), derive(sum, rel, temperatures)     restatements of the host functions
newton_tau(logits, yb)                                               the fp64 minimiser of the mean NLL of
                                                                     softmax(logits / tau), by Newton on beta = 1 / tau
                                                                     with bisection safeguards
"""
import math

import numpy as np

import eval_ref as E

NAN = float("nan")


def inv_t(tau):
    return np.float32(1.0) / np.float32(tau)


def record(row, x, y, values, is_percent, temperatures):
    """One row's K x 4 fields."""
    V, K = len(row), len(temperatures)
    out = np.full((K, 4), NAN)
    _, _, m_raw = E.weights(row)
    if m_raw == -np.inf or not (0 <= x < V and 0 <= y < V):
        return out
    if values is not None:
        v = np.asarray(values, dtype=np.float64)
        ch = v if is_percent else v - v[x]
        sg = (ch > 0).astype(np.int64) - (ch < 0).astype(np.int64)  # eval_ref.sign, over the vocabulary
    for k, tau in enumerate(temperatures):
        with np.errstate(all="ignore"):
            scaled = (np.asarray(row, dtype=np.float32) * inv_t(tau)).astype(np.float32)
        e, z, m = E.weights(scaled)
        S = math.fsum(e)
        out[k, 0] = -np.inf if z[y] == -np.inf else (0.0 if z[y] == m else float(z[y]) - float(m)) - math.log(S)
        if values is not None:
            for f, s in ((1, -1), (2, 0), (3, 1)):
                out[k, f] = math.fsum(e[sg == s]) / S
    return out


def records(logits, xb, yb, values=None, is_percent=False, temperatures=(1.0,), t_begin=0):
    logits = np.asarray(logits, dtype=np.float32)
    B, T, V = logits.shape
    rec = np.full((B, T, len(temperatures), 4), NAN)
    for b in range(B):
        for t in range(t_begin, T):
            rec[b, t] = record(logits[b, t], int(xb[b, t]), int(yb[b, t]), values, is_percent, temperatures)
    return rec


def realised(xb, yb, values, is_percent):
    xb, yb = np.asarray(xb), np.asarray(yb)
    out = np.full(xb.shape, NAN)
    if values is None:
        return out
    V = len(values)
    for idx in np.ndindex(*xb.shape):
        x, y = int(xb[idx]), int(yb[idx])
        if 0 <= x < V and 0 <= y < V:
            out[idx] = E.sign(float(values[y]), 0.0 if is_percent else float(values[x]), is_percent)
    return out


def tables(rec, t_begin=0, bins=10, realised=None):
    """Stage 2 on any records (the restatement's or the device's): every sum serial in fp64 from 0, a position's over
    b ascending, a cell over t ascending of the positions' own sums."""
    rec = np.asarray(rec, dtype=np.float64)
    B, T, K, _ = rec.shape
    tot, rel = np.zeros((K, 2)), np.zeros((K, 3, bins, 3))
    with np.errstate(all="ignore"):
        for t in range(t_begin, T):
            ptot, prel = np.zeros((K, 2)), np.zeros((K, 3, bins, 3))
            for b in range(B):
                for k in range(K):
                    r = rec[b, t, k]
                    if np.isnan(r[0]):
                        continue
                    ptot[k, 0] += 1.0
                    ptot[k, 1] += -r[0]
                    if np.isnan(r[1]):
                        continue
                    for d in range(3):
                        j = E.bin_of(r[1 + d], bins)
                        prel[k, d, j, 0] += 1.0
                        prel[k, d, j, 1] += r[1 + d]
                        prel[k, d, j, 2] += 1.0 if realised[b, t] == d - 1 else 0.0
            tot = tot + ptot
            rel = rel + prel
    return tot, rel


def fit(temperatures, rows, nll_sum):
    """(tau, k_star, at_bound): the rule of mmt_eval.fit_temperature's docstring, restated."""
    tau = np.asarray(temperatures, dtype=np.float64)
    K = len(tau)
    if not rows > 0:
        return NAN, -1, True
    with np.errstate(all="ignore"):
        mean = np.asarray(nll_sum, dtype=np.float64) / float(rows)
    mean = np.where(np.isfinite(mean), mean, np.inf)
    if not np.isfinite(mean).any():
        return NAN, -1, True
    ks = int(np.argmin(mean))  # the first minimum
    if K == 1 or ks in (0, K - 1):
        return float(tau[ks]), ks, True
    if not (np.isfinite(mean[ks - 1]) and np.isfinite(mean[ks + 1])):
        return float(tau[ks]), ks, False
    x = np.log(tau[ks - 1:ks + 2])
    y = mean[ks - 1:ks + 2]
    with np.errstate(all="ignore"):
        den = (x[1] - x[0]) * (y[1] - y[2]) - (x[1] - x[2]) * (y[1] - y[0])
    xs = x[1]
    if den != 0:
        with np.errstate(all="ignore"):
            v = x[1] - 0.5 * ((x[1] - x[0]) ** 2 * (y[1] - y[2]) - (x[1] - x[2]) ** 2 * (y[1] - y[0])) / den
        if np.isfinite(v) and x[0] <= v <= x[2]:
            xs = v
    return float(np.exp(xs)), ks, False


def derive(tot, rel, temperatures):
    tot, rel = np.asarray(tot, np.float64), np.asarray(rel, np.float64)
    temps = np.asarray(temperatures, np.float32)
    K = len(temps)
    with np.errstate(all="ignore"):
        nll = np.where(tot[:, 0] > 0, tot[:, 1] / np.where(tot[:, 0] > 0, tot[:, 0], 1.0), np.nan)
        ece = {}
        for d, name in enumerate(("down", "flat", "up")):
            n = rel[:, d, :, 0].sum(axis=1)
            gap = np.abs(rel[:, d, :, 1] - rel[:, d, :, 2]).sum(axis=1)
            ece[name] = np.where(n > 0, gap / np.where(n > 0, n, 1.0), np.nan)
    tau, ks, at_bound = fit(temps, tot[0, 0] if K else 0.0, tot[:, 1])
    one = [k for k in range(K) if temps[k] == np.float32(1.0)]
    return {"rows": int(tot[0, 0]) if K else 0, "nll": nll, "ece": ece, "tau": tau, "k_star": ks, "at_bound": at_bound,
            "k_one": one[0] if one else None}


def mean_nll(logits, yb, beta):
    """The fp64 mean NLL of softmax(beta * logits) at yb, with its first and second derivative in beta."""
    x = np.asarray(logits, dtype=np.float64)
    z = beta * x
    z = z - z.max(axis=1, keepdims=True)
    p = np.exp(z)
    p /= p.sum(axis=1, keepdims=True)
    xy = x[np.arange(len(x)), yb]
    mu = (p * x).sum(axis=1)
    var = (p * x * x).sum(axis=1) - mu * mu
    f = (np.log(np.exp(z).sum(axis=1)) - z[np.arange(len(x)), yb]).mean()
    return f, (mu - xy).mean(), var.mean()


def newton_tau(logits, yb, lo=1e-3, hi=1e3):
    """argmin over tau of the mean NLL: the NLL is convex in beta = 1 / tau, so the root of its derivative in
    [lo, hi] is the minimiser. Newton steps, bisection whenever a step leaves the bracket."""
    g_lo, g_hi = mean_nll(logits, yb, lo)[1], mean_nll(logits, yb, hi)[1]
    assert g_lo < 0 < g_hi, "the minimum is not inside the bracket"
    beta = 1.0
    for _ in range(200):
        _, g, h = mean_nll(logits, yb, beta)
        if g > 0:
            hi = beta
        else:
            lo = beta
        step = beta - g / h if h > 0 else NAN
        new = step if lo < step < hi else 0.5 * (lo + hi)
        if abs(new - beta) <= 1e-14 * beta:
            beta = new
            break
        beta = new
    return 1.0 / beta


def bracket_input():
    """The input of the bracket tests: 4096 rows, V = 16, logits N(0, 2^2), targets drawn from softmax(logits / 1.7)."""
    rng = np.random.default_rng(20240521)
    x = rng.normal(0.0, 2.0, size=(4096, 16)).astype(np.float32)
    z = x.astype(np.float64) / 1.7
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    u = rng.random(4096)
    yb = np.minimum((p.cumsum(axis=1) < u[:, None]).sum(axis=1), 15).astype(np.int64)
    return x, yb
