"""CPU restatement of the forecast rules (include/mmt.h: mmt_forecast_multi, mmt_pmf_stats), in fp64 numpy. Test
infrastructure only. It builds on sampling_ref.sample_rows for a row's kept set and its top-p margin, and on
evidence_ref.accumulate / weights for the path weights.

row_laws(x, t, k, p, delta)      the law of every row of x [R, V]: P fp64 [R, V] (zero rows where dead), `dead`, and
                                 for rows whose top-p margin is below delta (`amb`) the envelope [lo, hi] over the kept
                                 set and its two neighbours (one group fewer, one group more); elsewhere lo = hi = P.
                                 top-k keeps by exact comparisons (ties all kept): it is never ambiguous.
                                 `rel` [R, V]: the relative error allowed on P, expm1(lp_tol(V, ln P)).
mixture(laws, idx, a, ...)       rules 2 - 3 for one prompt whose path s is row idx[s] of the laws: pmf, envelope,
                                 bound, ess, live.
pmf_stats(q, ...)                mmt_pmf_stats for one stored fp32 row.

The input families of the GPU tests: the 64 rows of test_gpu_sample.make_rows(V) (N(0, 3^2) rows, tie rows, rows with
-inf / NaN entries, two rows with no finite logit), tiled into prompts by prompt_rows; evidence_ref.family
log-weights with prompt 1 shifted by -50 and, in prompt 2, -inf weights (log_weights)."""
import math

import numpy as np

import evidence_ref as E
import sampling_ref as R
from test_gpu_sample import delta as sample_delta
from test_gpu_sample import lp_tol, make_rows  # noqa: F401  (make_rows: the rows of the families)

SETTINGS = [(1.0, 0, 1.0), (0.8, 8, 1.0), (0.8, 0, 0.9), (1.3, 50, 0.5), (0.0, 7, 0.3)]
VS = [1, 5, 13, 64, 65, 900, 8193]
SAMPLES = [1, 2, 15, 16, 17, 64, 257, 1000]
PROMPTS = 3
EPS_W = 4 * 2.0 ** -23  # a weight: expf on the device (3 ulp, as test_gpu_sample takes it) against numpy's (1 ulp)
TINY = 2.0 ** -149  # the least fp32 subnormal: weights and results below it round to 0


def _law(z, kept):
    m = z.max()
    e = R._weights(z, m, kept)
    return e / e.sum()


def row_laws(x, t, k, p, delta=None):
    x = np.asarray(x, dtype=np.float32)
    Rn, V = x.shape
    delta = sample_delta(V) if delta is None else delta
    ref = R.sample_rows(x, t, k, p, 0, 0)
    P = np.zeros((Rn, V))
    lo, hi = np.zeros((Rn, V)), np.zeros((Rn, V))
    dead, amb = np.zeros(Rn, bool), np.zeros(Rn, bool)
    for r in range(Rn):
        z = R.scaled(x[r], t).astype(np.float64)
        if z.max() == -np.inf:
            dead[r] = True
            continue
        if t == 0:
            P[r, ref["token"][r]] = 1.0
            lo[r] = hi[r] = P[r]
            continue
        kept = ref["kept"][r]
        P[r] = _law(z, kept)
        lo[r] = hi[r] = P[r]
        if ref["margin_p"][r] < delta:
            amb[r] = True
            topk = np.ones(V, bool)
            if 0 < k < V:
                topk = z >= np.sort(z)[::-1][k - 1]
            vals = np.unique(z[topk])[::-1]  # the groups top-p chooses among, descending
            g = int(np.nonzero(vals == z[kept].min())[0][0])
            alts = [P[r]]
            if g > 0:
                alts.append(_law(z, topk & (z >= vals[g - 1])))
            if g + 1 < len(vals):
                alts.append(_law(z, topk & (z >= vals[g + 1])))
            lo[r], hi[r] = np.min(alts, axis=0), np.max(alts, axis=0)
    with np.errstate(all="ignore"):
        lnP = np.where(P > 0, np.log(np.where(P > 0, P, 1.0)), 0.0)
    rel = np.expm1(lp_tol(V, lnP))
    return {"P": P, "lo": lo, "hi": hi, "dead": dead, "amb": amb, "rel": rel, "V": V}


def path_weights(a, dead):
    """Rule 2 for one prompt: (w fp64 [S] holding fp32 values, ess, live)."""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = -np.inf
    a[dead] = -np.inf
    if a.max() == -np.inf:
        return np.zeros(len(a)), 0.0, 0
    w, _ = E.weights(a)
    W, Q = w.sum(), (w * w).sum()
    return w, W * W / Q, int((w > 0).sum())


def mixture(laws, idx, a=None, extra_rel=0.0):
    """One prompt: path s is row idx[s] of `laws`; a fp64 [S] (rule 1's sums) or None (no weights). Returns a dict:
    pmf, lo, hi (fp64 [V]), bound [V], ess, live, amb (ambiguous paths with weight). The bound, per element:
      sum_s (w_s / W) P_s(i) rel_s(i)          the row laws (delta(V) / lp_tol of the sampler tests)
      + q(i) (2 EPS_W + extra_rel)             the fp32 weights, in a ratio (0 without weights)
      + q(i) ((S + 16) 2^-53 + 2^-24) + 2^-149 the fp64 sums and the one fp32 rounding of the result."""
    idx = np.asarray(idx)
    S, V = len(idx), laws["V"]
    dead = laws["dead"][idx]
    weighted = a is not None
    w, ess, live = path_weights(np.zeros(S) if a is None else a, dead)
    out = {"ess": ess, "live": live, "amb": 0}
    if live == 0:
        z = np.zeros(V)
        out.update(pmf=z, lo=z, hi=z, bound=np.full(V, TINY))
        return out
    # the paths hold few distinct rows: the weight each distinct row carries, then one product per quantity
    c = np.bincount(idx, weights=w / w.sum(), minlength=len(laws["P"]))
    q = c @ laws["P"]
    err = c @ (laws["P"] * laws["rel"])
    wrel = (2 * EPS_W + extra_rel) if weighted else 0.0
    out.update(pmf=q, lo=c @ laws["lo"], hi=c @ laws["hi"],
               bound=err + q * (wrel + (S + 16) * 2.0 ** -53 + 2.0 ** -24) + TINY,
               amb=int((laws["amb"][idx] & (w > 0)).sum()))
    return out


def check_pmf(got, ref):
    """(largest error / bound over the elements, failing elements) of one prompt's fp32 row against `mixture`."""
    got = np.asarray(got, dtype=np.float64)
    over = np.maximum(np.maximum(ref["lo"] - got, got - ref["hi"]), 0.0)  # distance to the envelope
    ratio = over / ref["bound"]
    return float(ratio.max()), [int(i) for i in np.nonzero(~(ratio <= 1.0))[0]]


def prompt_rows(S, seed=0):
    """Which of the 64 family rows each path of the three prompts holds, int [3, S]. Prompt 0 holds no dead row;
    prompt 2 holds the dead rows 56 / 58 at every fifth path from path 0 on (so at S = 1 it is an all-dead prompt)."""
    rng = np.random.default_rng(7919 * seed + S)
    idx = rng.integers(0, 64, size=(PROMPTS, S))
    idx[0] = idx[0] % 48
    idx[2, 0::5] = 56
    idx[2, 5::10] = 58
    return idx


def log_weights(S, sigma, seed):
    """evidence_ref.family (prompt 1 shifted by -50), and -inf weights in prompt 2 at every seventh path from 1 on."""
    a = E.family(S, sigma, seed, prompts=PROMPTS)
    a[2, 1::7] = -np.inf
    return a


def brute_mixture(x, t, k, p, a=None):
    """The rule by brute force for tiny cases, no top-p margin logic: plain softmax over the kept set in Python
    floats, weights exp(a - max a) (not rounded to fp32). For the CPU tests of this restatement."""
    x = np.asarray(x, dtype=np.float32)
    S, V = x.shape
    laws = []
    for r in range(S):
        z = [float(v) for v in R.scaled(x[r], t)]
        if max(z) == -math.inf:
            laws.append(None)
            continue
        if t == 0:
            laws.append([1.0 if i == z.index(max(z)) else 0.0 for i in range(V)])
            continue
        keep = list(range(V))
        if 0 < k < V:
            thr = sorted(z, reverse=True)[k - 1]
            keep = [i for i in keep if z[i] >= thr]
        m = max(z)
        e = {i: math.exp(z[i] - m) if z[i] > -math.inf else 0.0 for i in keep}
        tot = math.fsum(e.values())
        if p < 1.0:
            pf = float(np.float32(p))
            chosen = None
            for v in sorted({z[i] for i in keep}, reverse=True):
                if chosen is None and (pf <= 0.0 or math.fsum(e[i] for i in keep if z[i] >= v) >= pf * tot):
                    chosen = v
            chosen = min(z[i] for i in keep) if chosen is None else chosen
            keep = [i for i in keep if z[i] >= chosen]
            tot = math.fsum(e[i] for i in keep)
        laws.append([e[i] / tot if i in keep else 0.0 for i in range(V)])
    aa = [0.0] * S if a is None else [(-math.inf if v != v else float(v)) for v in a]
    aa = [-math.inf if laws[s] is None else aa[s] for s in range(S)]
    mx = max(aa)
    if mx == -math.inf:
        return np.zeros(V), 0.0, 0
    w = [math.exp(v - mx) if v > -math.inf else 0.0 for v in aa]
    W = math.fsum(w)
    q = [math.fsum(w[s] * laws[s][i] for s in range(S) if w[s] > 0) / W for i in range(V)]
    return np.array(q), W * W / math.fsum(v * v for v in w), sum(1 for v in w if v > 0)


# ---- mmt_pmf_stats ----

QTOL = 1e-12  # a prefix sum this close to level * T (relative to T) may fall either side on the device


def direction_sign(v, origin_value, is_percent):
    """The reference's _get_direction_sign for numeric values."""
    ch = v if is_percent else v - origin_value
    return 1 if ch > 0 else -1 if ch < 0 else 0


def pmf_stats(q, values=None, is_percent=False, origin=None, levels=(0.05, 0.5, 0.95)):
    """One row. Returns (stats fp64 [8], qtok int [nq], alt int [nq]): alt[k] is the other token accepted for level k
    (the next token with mass) where a prefix sum lies within QTOL * T of the level, else qtok[k]."""
    q = np.asarray(q, dtype=np.float32)
    V, nq = len(q), len(levels)
    x = np.where(q > 0, q, 0).astype(np.float64)
    T = float(x.sum())
    st = np.full(8, np.nan)
    st[0] = T
    if not T > 0:
        return st, np.full(nq, -1), np.full(nq, -1)
    p = x / T
    pos = p > 0
    st[1] = float(-(p[pos] * np.log(p[pos])).sum())
    st[7] = float(x.max() / T)
    if values is not None:
        v = np.asarray(values, dtype=np.float64)
        st[2] = float((p * v).sum())
        st[3] = float((p * (v - st[2]) ** 2).sum())
        ok = is_percent or (origin is not None and 0 <= int(origin) < V)
        if ok:
            vo = 0.0 if is_percent else float(v[int(origin)])
            sign = np.array([direction_sign(float(t), vo, is_percent) for t in v])
            for k, sg in ((4, -1), (5, 0), (6, 1)):
                st[k] = float(x[(sign == sg) & pos].sum() / T)
    mass = np.nonzero(pos)[0]
    pref = np.cumsum(x)[mass]
    qtok, alt = np.zeros(nq, dtype=np.int64), np.zeros(nq, dtype=np.int64)
    for k, lv in enumerate(levels):
        target = lv * T
        j = min(int(np.searchsorted(pref, target, side="left")), len(mass) - 1)
        qtok[k] = alt[k] = mass[j]
        near = np.nonzero(np.abs(pref - target) <= QTOL * T)[0]
        if len(near):
            n0 = int(near[0])
            pair = (mass[n0], mass[min(n0 + 1, len(mass) - 1)])
            alt[k] = pair[1] if qtok[k] == pair[0] else pair[0]
    return st, qtok, alt


def stats_cases(V, seed=0):
    """The pmf rows of the GPU test at one V, fp32 [rows, V]: dense, point masses at both ends, two-point ties at the
    levels 0.5 / 0.05, zeros, an unnormalised row, a sparse row; and what they are for."""
    rng = np.random.default_rng(4000 + 31 * V + seed)
    rows, names = [], []

    def add(name, r):
        rows.append(np.asarray(r, dtype=np.float32))
        names.append(name)

    for n in range(40):  # many dense rows: the exact tie below is ambiguous by the rule, and the cap is 1 %
        d = rng.random(V) ** 3
        add(f"dense{n}", d / d.sum())
    for e in (0, V - 1):
        r = np.zeros(V)
        r[e] = 1.0
        add(f"point{e}", r)
    r = np.zeros(V)
    r[0] = r[V - 1] = 0.5
    add("tie_half", r if V > 1 else [1.0])
    r = np.zeros(V)
    r[0], r[V - 1] = 0.05, 0.95
    add("tie_low", r if V > 1 else [1.0])
    add("zeros", np.zeros(V))
    add("unnormalised", d * 3.7)
    r = np.where(rng.random(V) < 0.2, rng.random(V), 0.0)
    r[int(rng.integers(0, V))] = 0.5
    add("sparse", r / r.sum())
    return np.stack(rows), names


def stats_values(V, repeated=False, seed=0):
    """A sorted vocabulary of V values of both signs (N(0.75, 2^2): off centre, so a mean does not cancel to nothing);
    `repeated`: with runs of equal entries (and exact zeros)."""
    rng = np.random.default_rng(5000 + V + seed)
    v = np.sort(rng.normal(0.75, 2.0, size=V))
    if repeated:
        v = np.sort(np.round(v))
    return v
