"""CPU restatement of the horizon rules (include/mmt.h: mmt_horizon_stats), in fp64 numpy, on top of
evidence_ref.weights. Test infrastructure only.

paths(tok, values, is_percent, origin)   rule 1 for every row: x, hi, lo fp64 [R, N], d int [R, N], dead bool [R]. One
                                         IEEE operation per line, as the rule states it.
prompt(x, hi, lo, d, dead, a, levels, barriers)
                                         rules 2 - 5 for one prompt (a: fp64 [S] log-weights or None). Returns a dict:
    stats [N, 12], hit [N, nb], ess, live, w [S]
    qrow, qval [N, nq]                   the quantile row (local path index) and its x
    qalt, qalt_val [N, nq]               the neighbouring row with weight on the nearer side of the level, and its x
    margin [N, nq]                       |prefix - level W| / W at that nearer boundary (inf when there is none)
    bound [N, 12], hit_bound [N, nb]     the error allowed on each entry (below)

The bounds, derived from the rule and the number formats, not from any kernel's error:
  RTOL = 1e-12 stands for the fp64 roundings of a sum of up to 4096 terms in another order ((S + 16) 2^-53 < 5e-13), as
  in test_gpu_pmf_stats.py. A sum of terms of one sign gets RTOL times itself; the mean, whose terms have both signs,
  RTOL * sum w |x| / W. The variance is a function of the mean: about the exact mean m, sum w (x - m')^2 / W = var +
  (m' - m)^2, so the mean's own allowance enters squared, twice (the kernel's mean and this file's): RTOL var +
  2 mean_bound^2.
  With weights, a device expf may differ from numpy's by 4 ulp of fp32: every weight carries a relative error up to
  EPS = 4 * 2^-24. A ratio R = sum w f / sum w moves, to first order, by sum w delta (f - R) / W <= EPS sum w |f - R| /
  W <= 2 EPS sum w |f| / W; for a mass (f in {0, 1}) that is 2 EPS times the mass. So each weighted entry adds 2 EPS
  times its sum of magnitudes; the variance adds 2 EPS var (f = (x - m)^2) and the squared weighted mean bound; ess =
  W^2 / Q adds 4 EPS relative. min / max are order statistics of bit-exact x: no allowance.
  Quantiles: a prefix sum relative to W moves by at most 2 EPS = DELTA = 8 * 2^-24, so where the level lies at least
  DELTA from the nearest prefix boundary the row and its bits are exact; nearer, the row across that boundary is
  accepted too. Without weights the prefix sums are integers and nothing is ambiguous.

The input families of the GPU tests (case): tokens uniform in 0..V-1; sorted values rounded to 2 decimals (exact zeros
and repeats occur); log-weights from forecast_ref.log_weights (prompt 1 shifted by -50, -inf rows in prompt 2)."""
import functools
import math

import numpy as np

import evidence_ref as E
import forecast_ref as F

RTOL = 1e-12
EPS = 4 * 2.0 ** -24
DELTA = 8 * 2.0 ** -24
PROMPTS = 3
LEVELS = (0.05, 0.5, 0.95)
LEVELS16 = tuple((k + 0.5) / 16 for k in range(16))
BARRIERS = (0.5, -0.5, 3.0, -3.0)
BARRIERS8 = (0.5, -0.5, 3.0, -3.0, 1.0, -1.0, 8.0, -8.0)
SAMPLES = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4096]
VS = [1, 5, 900]
SIGMAS = [None, 0.3, 8.0]  # None: no weights


def steps_for(S):
    return [1, 2, 33] if S <= 65 else [1, 33]


def sign(a):
    return (a > 0).astype(np.int64) - (a < 0).astype(np.int64)


def paths(tok, values, is_percent, origin=None):
    tok = np.asarray(tok, dtype=np.int64)
    v = np.asarray(values, dtype=np.float64)
    R, N = tok.shape
    V = len(v)
    dead = ((tok < 0) | (tok >= V)).any(axis=1)
    vo = np.zeros(R)
    if not is_percent:
        o = np.asarray(origin, dtype=np.int64)
        dead |= (o < 0) | (o >= V)
        vo = v[np.clip(o, 0, V - 1)]
    vt = v[np.clip(tok, 0, V - 1)]
    x = np.zeros((R, N))
    d = np.zeros((R, N), dtype=np.int64)
    with np.errstate(all="ignore"):
        if is_percent:
            g = np.ones(R)
            for j in range(N):
                c = vt[:, j] / 100.0
                u = 1.0 + c
                g = g * u
                e = g - 1.0
                x[:, j] = e * 100.0
            d = sign(vt)
        else:
            prev = vo
            for j in range(N):
                x[:, j] = vt[:, j] - vo
                d[:, j] = sign(vt[:, j] - prev)
                prev = vt[:, j]
    dead |= ~np.isfinite(x).all(axis=1)
    x[dead] = 0.0
    hi = np.maximum.accumulate(np.maximum(x, 0.0), axis=1) if N else x.copy()
    lo = np.minimum.accumulate(np.minimum(x, 0.0), axis=1) if N else x.copy()
    return x, hi, lo, d, dead


def prompt(x, hi, lo, d, dead, a=None, levels=LEVELS, barriers=()):
    S, N = x.shape
    nq, nb = len(levels), len(barriers)
    weighted = a is not None
    w, ess, live = F.path_weights(np.zeros(S) if a is None else a, dead)
    out = {"ess": ess, "live": live, "w": w, "stats": np.full((N, 12), np.nan), "hit": np.full((N, nb), np.nan),
           "qrow": np.full((N, nq), -1), "qalt": np.full((N, nq), -1), "qval": np.full((N, nq), np.nan),
           "qalt_val": np.full((N, nq), np.nan), "margin": np.full((N, nq), math.inf),
           "bound": np.zeros((N, 12)), "hit_bound": np.zeros((N, nb))}
    if live == 0:
        return out
    W = w.sum()
    keep = np.nonzero(w > 0)[0]
    wk = w[keep]
    extra = 2 * EPS if weighted else 0.0
    st, bd = out["stats"], out["bound"]
    for j in range(N):
        xj, hj, lj, dj = x[keep, j], hi[keep, j], lo[keep, j], d[keep, j]
        mean = (wk * xj).sum() / W
        mabs = (wk * np.abs(xj)).sum() / W
        var = (wk * (xj - mean) ** 2).sum() / W
        st[j, 0], bd[j, 0] = mean, (RTOL + extra) * mabs
        st[j, 1], bd[j, 1] = var, (RTOL + extra) * var + 2 * bd[j, 0] ** 2
        for k, m in ((2, xj < 0), (3, xj == 0), (4, xj > 0), (5, dj < 0), (6, dj == 0), (7, dj > 0)):
            st[j, k] = wk[m].sum() / W
            bd[j, k] = (RTOL + extra) * st[j, k]
        st[j, 8], bd[j, 8] = (wk * hj).sum() / W, (RTOL + extra) * (wk * hj).sum() / W
        st[j, 9], bd[j, 9] = (wk * lj).sum() / W, (RTOL + extra) * (wk * -lj).sum() / W
        st[j, 10], st[j, 11] = xj.min(), xj.max()
        for k, u in enumerate(barriers):
            out["hit"][j, k] = wk[hj >= u].sum() / W if u > 0 else wk[lj <= u].sum() / W
            out["hit_bound"][j, k] = (RTOL + extra) * out["hit"][j, k]
        order = np.lexsort((keep, xj))  # (x, s) ascending
        rows, xs = keep[order], xj[order]
        pref = np.cumsum(wk[order])
        n = len(rows)
        for k, lv in enumerate(levels):
            target = lv * W
            i = min(int(np.searchsorted(pref, target, side="left")), n - 1)
            out["qrow"][j, k], out["qval"][j, k] = rows[i], xs[i]
            out["qalt"][j, k], out["qalt_val"][j, k] = rows[i], xs[i]
            if n > 1:
                below = target - pref[i - 1] if i > 0 else math.inf  # towards the previous row with weight
                above = pref[i] - target if i < n - 1 else math.inf  # towards the next one
                alt = i - 1 if below <= above else i + 1
                out["margin"][j, k] = abs(min(below, above)) / W
                out["qalt"][j, k], out["qalt_val"][j, k] = rows[alt], xs[alt]
    return out


def values_for(V, seed=0):
    """A sorted vocabulary of V values of both signs rounded to 2 decimals (N(0.1, 1.5^2)): exact zeros and repeats
    occur at V = 900; + 0.0 turns a rounded -0.0 into +0.0."""
    rng = np.random.default_rng(6000 + 13 * V + seed)
    v = np.sort(np.round(rng.normal(0.1, 1.5, size=V), 2)) + 0.0
    if V >= 5:
        v[V // 2] = 0.0  # an exact zero at every size but V = 1
        v = np.sort(v)
    return v


@functools.lru_cache(maxsize=None)
def case(S, N, V, sigma, seed=0, levels=LEVELS, barriers=BARRIERS):
    """One GPU test case, computed once and shared: tokens int64 [2][3 S, N] and origins for a percent problem (0) and
    a value problem (1), the values, the log-weights (None without) and the reference of every (problem, prompt)."""
    rng = np.random.default_rng(900001 * seed + 7919 * S + 131 * N + V)
    R = PROMPTS * S
    tok = [rng.integers(0, V, size=(R, N)), rng.integers(0, V, size=(R, N))]
    origin = rng.integers(0, V, size=R)
    v = values_for(V, seed)
    a = None if sigma is None else F.log_weights(S, sigma, seed).reshape(-1)
    ref = []
    for p in range(2):
        pq = paths(tok[p], v, p == 0, origin)
        ref.append([prompt(*[t[b * S:(b + 1) * S] for t in pq], None if a is None else a[b * S:(b + 1) * S], levels,
                           barriers) for b in range(PROMPTS)])
    return {"tok": tok, "origin": origin, "values": v, "logw": a, "ref": ref, "S": S, "N": N, "V": V}


def ambiguous(ref_prompts):
    """(ambiguous, all) (prompt, step, level) triples of one problem's reference."""
    amb = sum(int((r["margin"] < DELTA).sum()) for r in ref_prompts)
    return amb, sum(r["margin"].size for r in ref_prompts)


def cap(triples):
    return max(1, int(0.02 * triples))


def check(got, ref, weighted, what=""):
    """One prompt of one problem against `prompt`: got = dict(stats [N, 12], qval, qrow [N, nq], hit [N, nb], ess,
    live). Asserts the bounds; returns (ambiguous triples, largest error / bound over stats and hit)."""
    N = ref["stats"].shape[0]
    assert int(got["live"]) == ref["live"], (what, got["live"], ref["live"])
    if ref["live"] == 0:
        assert got["ess"] == 0.0 and np.isnan(got["stats"]).all() and np.isnan(got["qval"]).all(), what
        assert (got["qrow"] == -1).all() and np.isnan(got["hit"]).all(), what
        return 0, 0.0
    etol = (RTOL + (4 * EPS if weighted else 0.0)) * ref["ess"]
    assert abs(got["ess"] - ref["ess"]) <= etol, (what, got["ess"], ref["ess"])
    worst = 0.0
    if N == 0:
        return 0, worst
    assert np.array_equal(got["stats"][:, 10:].view(np.int64), ref["stats"][:, 10:].view(np.int64)), (what, "min/max")
    err = np.abs(got["stats"][:, :10] - ref["stats"][:, :10])
    bad = ~(err <= ref["bound"][:, :10])
    assert not bad.any(), (what, "stats (step, entry)", np.argwhere(bad)[:4], got["stats"][:, :10][bad][:4],
                           ref["stats"][:, :10][bad][:4], ref["bound"][:, :10][bad][:4])
    herr = np.abs(got["hit"] - ref["hit"])
    assert (herr <= ref["hit_bound"]).all(), (what, "hit", got["hit"], ref["hit"])
    with np.errstate(all="ignore"):
        for e, b in ((err, ref["bound"][:, :10]), (herr, ref["hit_bound"])):
            r = np.where(e > 0, e / np.where(b > 0, b, 1.0), 0.0)
            worst = max(worst, float(r.max()) if r.size else 0.0)
    clear = ref["margin"] >= DELTA if weighted else np.ones_like(ref["margin"], dtype=bool)
    exact = (got["qrow"] == ref["qrow"]) & (got["qval"].view(np.int64) == ref["qval"].view(np.int64))
    other = (got["qrow"] == ref["qalt"]) & (got["qval"].view(np.int64) == ref["qalt_val"].view(np.int64))
    ok = exact | (~clear & other)
    assert ok.all(), (what, "quantiles", np.argwhere(~ok)[:4], got["qrow"][~ok][:4], ref["qrow"][~ok][:4],
                      ref["margin"][~ok][:4])
    return int((~clear).sum()), worst


def brute(tok, values, is_percent, origin, a, levels, barriers):
    """One prompt by brute force in Python floats: serial sums in row order, a sort of Python tuples, weights
    exp((float) (a - max a)) (the exponent rounded to fp32 as the rule says, the weight not). Returns (stats [N][12], qrow [N][nq], qval, hit [N][nb], live)."""
    S, N, V = len(tok), len(tok[0]), len(values)
    v = [float(t) for t in values]
    rows = []
    for s in range(S):
        ok = all(0 <= int(t) < V for t in tok[s]) and (is_percent or 0 <= int(origin[s]) < V)
        xs, his, los, ds = [], [], [], []
        if ok:
            g, h, l = 1.0, 0.0, 0.0
            prev = None if is_percent else v[int(origin[s])]
            for j in range(N):
                t = v[int(tok[s][j])]
                if is_percent:
                    g = g * (1.0 + t / 100.0)
                    x = (g - 1.0) * 100.0
                    dd = (t > 0) - (t < 0)
                else:
                    x = t - v[int(origin[s])]
                    dd = (t - prev > 0) - (t - prev < 0)
                    prev = t
                ok = ok and math.isfinite(x)
                h, l = max(h, x), min(l, x)
                xs.append(x), his.append(h), los.append(l), ds.append(dd)
        rows.append((ok, xs, his, los, ds))
    aa = [0.0 if a is None else (-math.inf if a[s] != a[s] else float(a[s])) for s in range(S)]
    aa = [aa[s] if rows[s][0] else -math.inf for s in range(S)]
    mx = max(aa)
    if mx == -math.inf:
        return None
    w = [math.exp(float(np.float32(t - mx))) if t > -math.inf else 0.0 for t in aa]
    W = math.fsum(w)
    liv = [s for s in range(S) if w[s] > 0]
    stats, qrow, qval, hit = [], [], [], []
    for j in range(N):
        x = {s: rows[s][1][j] for s in liv}
        mean = math.fsum(w[s] * x[s] for s in liv) / W
        st = [mean, math.fsum(w[s] * (x[s] - mean) ** 2 for s in liv) / W]
        st += [math.fsum(w[s] for s in liv if c(x[s])) / W for c in (lambda t: t < 0, lambda t: t == 0, lambda t: t > 0)]
        st += [math.fsum(w[s] for s in liv if rows[s][4][j] == sg) / W for sg in (-1, 0, 1)]
        st += [math.fsum(w[s] * rows[s][2][j] for s in liv) / W, math.fsum(w[s] * rows[s][3][j] for s in liv) / W]
        st += [min(x.values()), max(x.values())]
        stats.append(st)
        hit.append([math.fsum(w[s] for s in liv if (rows[s][2][j] >= u if u > 0 else rows[s][3][j] <= u)) / W
                    for u in barriers])
        order = sorted((x[s], s) for s in liv)
        qr, qv = [], []
        for lv in levels:
            acc, pick = 0.0, order[-1]
            for xv, s in order:
                acc += w[s]
                if acc >= lv * W:
                    pick = (xv, s)
                    break
            qr.append(pick[1]), qv.append(pick[0])
        qrow.append(qr), qval.append(qv)
    return stats, qrow, qval, hit, len(liv)
