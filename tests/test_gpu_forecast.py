"""mmt_forecast_multi (csrc/mmt_forecast.hip) through the C ABI, against the fp64 restatement tests/forecast_ref.py.

Inputs: the 64 rows of test_gpu_sample.make_rows(V) tiled into three prompts of `samples` paths
(forecast_ref.prompt_rows: prompt 0 without dead rows, prompt 2 with the two rows that hold no finite logit), the
sampler tests' settings as five problems of ONE launch over the same logits, and evidence_ref.family log-weights
(prompt 1 shifted by -50, -inf weights in prompt 2).

The bound, per element i of a prompt's row, from its sources (forecast_ref.mixture computes it from the reference's
own numbers, never from the device's):
  * the row laws. P_r(i) = e_i / S_r with e_i an fp32 expf of an fp32 difference and S_r an fp64 sum of such weights:
    the sampler tests' lp_tol(V, ln P) is the bound on ln P they hold the kernel to (delta(V) for S_r, 2^-23 (|ln P| +
    ln V + 1) for the difference and expf), so P is off by at most the relative expm1(lp_tol(V, ln P_r(i))); in the
    mixture that is sum_s (w_s / W) P_r(i) expm1(lp_tol).
  * the weights. w_s is an fp32 expf of d_s = (float)(a_s - mx); device and restatement form the same d_s (a_s is a
    serial fp64 sum in one order) and differ in expf: 3 ulp on the device (as test_gpu_sample takes it) and 1 ulp in
    numpy, EPS_W = 4 * 2^-23 relative. q is a ratio of two sums of weights: 2 EPS_W q(i). Nothing without weights.
  * the fp64 sums (samples terms in a tree of depth <= samples / 16 + 16, one division) and the ONE fp32 rounding of the
    result: q(i) ((samples + 16) 2^-53 + 2^-24), plus 2^-149, the least fp32 subnormal, below which weights and results
    round to zero.
A row whose top-p margin is below delta(V) may keep one group more or fewer than the restatement (the sampler tests'
ambiguous rows; top-k compares exactly and ties are all kept, so it adds none): for those rows the restatement gives
the envelope [lo, hi] over the neighbouring kept sets and the bound is taken from the envelope. At most 5 % of a
family's rows may be ambiguous (test_forecast_ref_cpu.py shows the families stay within it).

Largest error / bound per shape, as printed by test_forecast_matches_the_rule on an MI355X: DESIGN.md §6."""
import ctypes

import numpy as np
import pytest
import torch

import evidence_ref as E
import forecast_ref as F
import mmt_lib as ML
import mmt_sample as MS
from test_gpu_sample import SEED, launch as sample_launch, lp_tol

pytestmark = pytest.mark.gpu

GUARD = -7.0
_laws, _dev_rows = {}, {}


def laws_for(V, setting):
    """The reference laws of the 64 family rows, computed once per (V, setting) and shared (read only)."""
    if (V, setting) not in _laws:
        _laws[(V, setting)] = F.row_laws(F.make_rows(V), *setting)
    return _laws[(V, setting)]


def dev_rows(V):
    if V not in _dev_rows:
        _dev_rows[V] = torch.from_numpy(F.make_rows(V).copy()).cuda()
    return _dev_rows[V]


def run(xd, B, S, settings, logw=None, lps=(), lp_stride=None, j0=0, j1=0, poison=False, pad=3, row_stride=None,
        raw=False, logw_out=None):
    """One mmt_forecast_multi over len(settings) problems that all read xd [B * S, V]. Outputs sit inside guard rows
    and columns, which are checked. Returns (pmf [P, B, V], ess [P, B], live [P, B]) as numpy, or with raw the
    status and the untouched-flag."""
    P, V = len(settings), xd.shape[1]
    dev = xd.device
    L = ML.lib()
    pmf = torch.full((P, B + 2, V + pad), GUARD, dtype=torch.float32, device=dev)
    ess = torch.full((P, B + 2), GUARD, dtype=torch.float64, device=dev)
    live = torch.full((P, B + 2), -7, dtype=torch.int32, device=dev)
    fl = MS.ForecastLaunch([V] * P, [MS.check_settings(*s) for s in settings], [V + pad] * P,
                           [t.data_ptr() for t in lps], [lp_stride or (t.shape[1] if len(lps) else 0) for t in lps])
    for p in range(P):
        fl.logits[p] = xd.data_ptr()
        fl.row_stride[p] = row_stride or V
        fl.pmf[p] = pmf[p, 1, 1:].data_ptr()
        fl.ess[p] = ess[p, 1:].data_ptr()
        fl.live[p] = live[p, 1:].data_ptr()
    nbytes = fl.scratch_bytes(L, B, S)
    scratch = torch.full((nbytes + 64,), 0xFF if poison else 0, dtype=torch.uint8, device=dev)  # 0xFF..: NaN bytes
    rc = L.mmt_forecast_multi(ML.stream_ptr(dev), P, B, S, fl.V, fl.logits, fl.row_stride, fl.temperature, fl.top_k,
                              fl.top_p, fl.pmf, fl.pmf_stride, fl.G, fl.lp, fl.lp_stride, j0, j1,
                              logw.data_ptr() if logw is not None else None,
                              logw_out.data_ptr() if logw_out is not None else None, fl.ess, fl.live,
                              scratch.data_ptr(), nbytes)
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == (0xFF if poison else 0)).all()), "wrote past the scratch"
    body = pmf[:, 1:B + 1, 1:V + 1]
    pmf_guard = pmf.clone()
    pmf_guard[:, 1:B + 1, 1:V + 1] = GUARD
    untouched = bool((pmf_guard == GUARD).all()) and bool((ess[:, 0] == GUARD).all()) and bool(
        (ess[:, B + 1] == GUARD).all()) and bool((live[:, 0] == -7).all()) and bool((live[:, B + 1] == -7).all())
    if raw:
        return rc, untouched and bool((body == GUARD).all()) and bool((ess == GUARD).all())
    assert rc == 0
    assert untouched, "wrote outside its pmf rows / ess / live"
    return body.cpu().numpy(), ess[:, 1:B + 1].cpu().numpy(), live[:, 1:B + 1].cpu().numpy()


def tiled(V, S, seed=0):
    idx = F.prompt_rows(S, seed)
    return idx, dev_rows(V)[torch.from_numpy(idx.ravel()).cuda()].contiguous()


def check_case(V, S, got, idx, a, what, extra_rel=0.0):
    """Every problem and prompt of one launch against the restatement. Returns the largest error / bound."""
    pmf, ess, live = got
    worst = 0.0
    for p, setting in enumerate(F.SETTINGS):
        laws = laws_for(V, setting)
        assert laws["amb"].sum() <= 0.05 * 64, (V, setting)
        for b in range(F.PROMPTS):
            ref = F.mixture(laws, idx[b], None if a is None else a[b], extra_rel)
            ratio, bad = F.check_pmf(pmf[p, b], ref)
            worst = max(worst, ratio)
            assert not bad, (what, V, S, setting, b, ratio, bad[:5])
            assert int(live[p, b]) == ref["live"], (what, V, S, setting, b)
            assert abs(ess[p, b] - ref["ess"]) <= 4 * F.EPS_W * ref["ess"], (what, V, S, setting, b)
            if ref["live"] == 0:
                assert not pmf[p, b].any()
            elif ref["amb"] == 0:
                assert abs(float(pmf[p, b].astype(np.float64).sum()) - 1.0) <= 1e-5
    return worst


@pytest.mark.parametrize("V", F.VS)
def test_forecast_matches_the_rule(V):
    """Every samples count, without weights and with log-weights N(0, 0.3^2) and N(0, 8^2) handed in as logw."""
    for S in F.SAMPLES:
        idx, xd = tiled(V, S)
        for sigma in (None, 0.3, 8.0):
            a = None if sigma is None else F.log_weights(S, sigma, 1)
            logw = None if a is None else torch.from_numpy(a.ravel().copy()).cuda()
            got = run(xd, F.PROMPTS, S, F.SETTINGS, logw=logw)
            worst = check_case(V, S, got, idx, a, f"sigma={sigma}")
            print(f"forecast V={V} samples={S} sigma={sigma}: max error / bound {worst:.3f}")


@pytest.mark.parametrize("V", [13, 900])
def test_weights_from_logprob_columns(V):
    """The weights as generate hands them in: two fp32 matrices with a row stride, the columns [1, 3) of four, plus
    logw; NaN entries count as -inf. The restatement's a_s is evidence_ref.accumulate's serial sum."""
    S, N, stride = 17, 4, 6
    idx, xd = tiled(V, S, seed=3)
    rng = np.random.default_rng(V)
    R = F.PROMPTS * S
    lps = [np.full((R, stride), 99.0, dtype=np.float32) for _ in range(2)]  # a huge pad: reading it would show
    for m in lps:
        m[:, :N] = -rng.random((R, N)).astype(np.float32) * 3
    lps[0][5, 1] = np.nan
    lps[1][S + 2, 2] = -np.inf
    logw = -rng.random(R) * 2
    a = E.accumulate(logw, [m[:, :N] for m in lps], 1, 3).reshape(F.PROMPTS, S)
    got = run(xd, F.PROMPTS, S, F.SETTINGS, logw=torch.from_numpy(logw).cuda(),
              lps=[torch.from_numpy(m).cuda() for m in lps], lp_stride=stride, j0=1, j1=3)
    print(f"forecast columns V={V}: max error / bound {check_case(V, S, got, idx, a, 'columns'):.3f}")
    # carried from step to step through logw_out, one column a call, the sums are the one-shot sums bit for bit
    carry = [torch.from_numpy(logw).cuda(), torch.full((R,), 7.0, dtype=torch.float64).cuda()]
    for j in (1, 2):
        step = run(xd, F.PROMPTS, S, F.SETTINGS, logw=carry[0], lps=[torch.from_numpy(m).cuda() for m in lps],
                   lp_stride=stride, j0=j, j1=j + 1, logw_out=carry[1])
        carry.reverse()
    assert np.array_equal(bits(carry[0].cpu().numpy()), bits(a.ravel()))
    for x, y in zip(step, got):
        assert np.array_equal(bits(x), bits(y))
    # an empty column range leaves logw alone
    a0 = E.accumulate(logw, [], 0, 0).reshape(F.PROMPTS, S)
    got = run(xd, F.PROMPTS, S, F.SETTINGS, logw=torch.from_numpy(logw).cuda(),
              lps=[torch.from_numpy(m).cuda() for m in lps], lp_stride=stride, j0=2, j1=2)
    check_case(V, S, got, idx, a0, "empty range")


@pytest.mark.parametrize("V", [13, 900, 8193])
def test_consistent_with_the_sampler(V):
    """With samples = 1 and no weights the pmf is the sampler's own distribution of the row: every token mmt_sample
    draws over 64 positions has pmf > 0, and log(pmf[tok]) meets the log-probability it reports within lp_tol plus
    the pmf's one fp32 rounding."""
    xd = dev_rows(V)
    pmf, ess, live = run(xd, 64, 1, F.SETTINGS)
    for p, (t, k, tp) in enumerate(F.SETTINGS):
        for pos in range(64):
            tok, lp, _, rc = sample_launch(xd, V, 64, t, k, tp, pos=pos)
            assert rc == 0
            tok, lp = tok.numpy(), lp.numpy().astype(np.float64)
            q = pmf[p, np.arange(64), tok].astype(np.float64)
            alive = ~np.isnan(lp)
            assert list(np.nonzero(~alive)[0]) == [56, 58] and not pmf[p, [56, 58]].any()
            assert np.all(q[alive] > 0), (V, t, k, tp, pos)
            if t == 0.0:  # greedy: the law is a point mass, while the sampler reports the raw log-softmax there
                assert np.all(q[alive] == 1.0)
                continue
            err = np.abs(np.log(q[alive]) - lp[alive])
            assert np.all(err <= lp_tol(V, lp[alive]) + 2.0 ** -23), (V, t, k, tp, pos, float(err.max()))
        assert np.array_equal(live[p], np.where(np.isin(np.arange(64), [56, 58]), 0, 1))
        assert np.array_equal(ess[p], live[p].astype(np.float64))


def bits(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)


@pytest.mark.parametrize("V,S", [(65, 17), (900, 257), (8193, 16)])
@pytest.mark.parametrize("weighted", [False, True])
def test_exact_properties(V, S, weighted):
    """Two runs agree bit for bit, also over a scratch prefilled with NaN bytes; a prompt alone gives the bits it gives
    in company; a problem alone gives the bits it gives among eight others (nine problems: two chunks)."""
    idx, xd = tiled(V, S, seed=5)
    a = F.log_weights(S, 2.0, 3) if weighted else None
    logw = torch.from_numpy(a.ravel().copy()).cuda() if weighted else None
    one = run(xd, F.PROMPTS, S, F.SETTINGS, logw=logw)
    two = run(xd, F.PROMPTS, S, F.SETTINGS, logw=logw, poison=True)
    for x, y in zip(one, two):
        assert np.array_equal(bits(x), bits(y))
    for b in range(F.PROMPTS):
        alone = run(xd[b * S:(b + 1) * S], 1, S, F.SETTINGS, logw=None if logw is None else logw[b * S:(b + 1) * S])
        for x, y in zip(one, alone):
            assert np.array_equal(bits(x[:, b]), bits(y[:, 0])), (V, S, b)
    nine = F.SETTINGS[:4] + [(0.7, 3, 0.95), (1.0, 0, 0.2), (2.0, 0, 1.0), (0.5, 1, 1.0)] + F.SETTINGS[4:]
    many = run(xd, F.PROMPTS, S, nine, logw=logw, poison=True)
    for p, q in ((0, 0), (3, 3), (4, 8)):
        for x, y in zip(one, many):
            assert np.array_equal(bits(x[p]), bits(y[q])), (V, S, p)
    solo = run(xd, F.PROMPTS, S, [nine[6]], logw=logw)
    for x, y in zip(solo, many):
        assert np.array_equal(bits(x[0]), bits(y[6]))


def test_problems_of_both_row_variants_in_one_call():
    """V <= 8192 rows (LDS) and larger ones (re-read) in one call are two law launches; each problem keeps the bits it
    has alone. The problems read one [R, 8193] buffer, the small one its first 900 columns (row stride 8193)."""
    S = 16
    idx, xd = tiled(8193, S, seed=2)
    big = run(xd, F.PROMPTS, S, [F.SETTINGS[2]])
    small = run(xd[:, :900], F.PROMPTS, S, [F.SETTINGS[2]], row_stride=8193)
    L, dev = ML.lib(), xd.device
    B = F.PROMPTS
    outs = [torch.full((B, v), GUARD, dtype=torch.float32, device=dev) for v in (900, 8193, 900)]
    fl = MS.ForecastLaunch([900, 8193, 900], [MS.check_settings(*F.SETTINGS[2])] * 3, [900, 8193, 900])
    for p in range(3):
        fl.logits[p], fl.row_stride[p], fl.pmf[p] = xd.data_ptr(), 8193, outs[p].data_ptr()
    nbytes = fl.scratch_bytes(L, B, S)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fl.run(L, ML.stream_ptr(dev), B, S, 0, 0, 0, scratch.data_ptr(), nbytes)
    torch.cuda.synchronize()
    assert np.array_equal(bits(outs[0].cpu().numpy()), bits(small[0][0]))
    assert np.array_equal(bits(outs[2].cpu().numpy()), bits(small[0][0]))
    assert np.array_equal(bits(outs[1].cpu().numpy()), bits(big[0][0]))


def test_equal_rows_dead_rows_and_cut_weights():
    """Equal rows with equal weights give the samples = 1 pmf within one fp32 ulp; a dead row and a -inf weight
    contribute nothing (one live path left: the samples = 1 bits); an all-dead prompt gives zeros, ess 0, live 0."""
    V = 900
    base = dev_rows(V)
    single, _, _ = run(base, 64, 1, F.SETTINGS)
    for S in (2, 17, 257):
        rows = torch.tensor([5] * S + [20] * S + [49] * S)
        for logw in (None, torch.full((3 * S,), -3.25, dtype=torch.float64).cuda()):
            pmf, ess, live = run(base[rows.cuda()].contiguous(), 3, S, F.SETTINGS, logw=logw)
            for b, r in enumerate((5, 20, 49)):
                want = single[:, r].astype(np.float64)
                ulp = np.spacing(np.abs(single[:, r])).astype(np.float64)
                assert np.all(np.abs(pmf[:, b].astype(np.float64) - want) <= ulp), (S, r)
                assert np.all(live[:, b] == S) and np.allclose(ess[:, b], S, rtol=1e-12)
    rows = torch.tensor([5, 56, 7, 58, 56, 58, 56, 56, 20, 58, 5, 56])  # S = 4: one live path, none, two (one cut)
    a = np.zeros(12)
    a[2] = -np.inf
    a[10] = np.nan
    pmf, ess, live = run(base[rows.cuda()].contiguous(), 3, 4, F.SETTINGS, logw=torch.from_numpy(a).cuda())
    assert np.array_equal(bits(pmf[:, 0]), bits(single[:, 5])) and np.all(live[:, 0] == 1) and np.all(ess[:, 0] == 1)
    assert not pmf[:, 1].any() and np.all(live[:, 1] == 0) and np.all(ess[:, 1] == 0)
    assert np.array_equal(bits(pmf[:, 2]), bits(single[:, 20])) and np.all(live[:, 2] == 1)
    pmf, ess, live = run(base[rows.cuda()].contiguous(), 3, 4, F.SETTINGS)  # without weights: paths 5 and 7 both count
    assert np.all(live[:, 0] == 2) and np.all(live[:, 1] == 0) and np.all(live[:, 2] == 2) and not pmf[:, 1].any()


@pytest.mark.parametrize("V,S", [(13, 64), (900, 1000)])
def test_a_weight_shift_moves_nothing_beyond_the_bound(V, S):
    """Every prompt's log-weights shifted by -50 against the restatement of the UNSHIFTED ones. The shift changes
    a_s - mx by fp64 roundings only, but those can move its fp32 rounding by one ulp: 2^-23 |d_s| relative on a
    weight, |d_s| <= 104 where a weight is not zero, in a ratio: extra_rel = 2^-22 * 104."""
    idx, xd = tiled(V, S, seed=4)
    a = F.log_weights(S, 2.0, 6)
    shifted = torch.from_numpy((a - 50.0).ravel().copy()).cuda()
    got = run(xd, F.PROMPTS, S, F.SETTINGS, logw=shifted)
    worst = check_case(V, S, got, idx, a, "shift", extra_rel=2.0 ** -22 * 104)
    print(f"forecast shift V={V} samples={S}: max error / bound {worst:.3f}")


def test_many_samples_without_weights_and_the_public_wrapper():
    """Without weights any samples count runs (5000 paths a prompt); with weights 4096 is the cap. The public
    forecast_multi gives the C entry's bits."""
    V, S = 5, 5000
    idx, xd = tiled(V, S, seed=9)
    got = run(xd, F.PROMPTS, S, F.SETTINGS)
    check_case(V, S, got, idx, None, "5000")
    ts, ks, ps = zip(*F.SETTINGS)
    pmfs, ess, live = MS.forecast_multi([xd] * len(F.SETTINGS), samples=S, temperature=list(ts), top_k=list(ks),
                                        top_p=list(ps))
    for p in range(len(F.SETTINGS)):
        assert np.array_equal(bits(pmfs[p].cpu().numpy()), bits(got[0][p]))
        assert np.array_equal(live[p].cpu().numpy(), got[2][p])
    logw = torch.zeros(F.PROMPTS * S, dtype=torch.float64, device="cuda")
    rc, clean = run(xd, F.PROMPTS, S, F.SETTINGS, logw=logw, raw=True)
    assert rc == -2 and clean  # MMT_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        MS.forecast_multi([xd], samples=S, logw=logw)
    idx, xd = tiled(13, 17)
    a = F.log_weights(17, 2.0, 2)
    lw = torch.from_numpy(a.ravel().copy()).cuda()
    got = run(xd, F.PROMPTS, 17, F.SETTINGS[:1], logw=lw)
    pmfs, ess, live = MS.forecast_multi([xd], samples=17, logw=lw)
    assert np.array_equal(bits(pmfs[0].cpu().numpy()), bits(got[0][0]))
    assert np.array_equal(bits(ess[0].cpu().numpy()), bits(got[1][0]))


def test_refusals_write_nothing():
    V, B, S = 13, 3, 4
    xd = torch.zeros(B * S, V, dtype=torch.float32, device="cuda")
    dev = xd.device
    L = ML.lib()
    nan = float("nan")
    lpm = torch.zeros(B * S, 4, dtype=torch.float32, device=dev)
    logw = torch.zeros(B * S, dtype=torch.float64, device=dev)

    def call(count=1, batch=B, samples=S, V_=V, stride=V, t=1.0, k=0, p=1.0, logits=xd, pmf_stride=V + 3, wcount=0,
             lp=None, lp_stride=4, j0=0, j1=0, lw=None, scratch="ok", short=0, arrays=True, out_w=None):
        pmf = torch.full((B + 2, V + 3), GUARD, dtype=torch.float32, device=dev)
        ess = torch.full((B,), GUARD, dtype=torch.float64, device=dev)
        need = max(int(L.mmt_forecast_scratch_bytes(1, B, S)), 16)
        sc = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device=dev)
        i32, i64, f32, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
        sptr = {"ok": sc.data_ptr(), "null": None, "odd": sc.data_ptr() + 4}[scratch]
        rc = L.mmt_forecast_multi(
            ML.stream_ptr(dev), count, batch, samples, (i32 * 1)(V_) if arrays else None,
            (vp * 1)(logits.data_ptr() if logits is not None else None), (i64 * 1)(stride), (f32 * 1)(t), (i32 * 1)(k),
            (f32 * 1)(p), (vp * 1)(pmf[1, 1:].data_ptr()), (i64 * 1)(pmf_stride), wcount,
            (vp * 1)(lp.data_ptr() if lp is not None else None), (i64 * 1)(lp_stride), j0, j1,
            lw.data_ptr() if lw is not None else None, out_w.data_ptr() if out_w is not None else None,
            (vp * 1)(ess.data_ptr()), None, sptr, need - short)
        torch.cuda.synchronize()
        clean = bool((pmf == GUARD).all()) and bool((ess == GUARD).all()) and bool((sc == 0x5A).all())
        return rc, clean

    invalid = [dict(samples=0), dict(samples=-2), dict(batch=-1), dict(count=-1), dict(batch=2 ** 20, samples=2 ** 11),
               dict(V_=0), dict(stride=V - 1), dict(t=-0.5), dict(t=nan), dict(k=-1), dict(p=nan), dict(logits=None),
               dict(pmf_stride=V - 1), dict(wcount=1, lp=lpm, lp_stride=2, j0=0, j1=3), dict(wcount=9, lp=lpm),
               dict(wcount=1, lp=None, j0=0, j1=2), dict(wcount=1, lp=lpm, j0=2, j1=1), dict(j0=-1),
               dict(scratch="null"), dict(scratch="odd"), dict(short=8), dict(arrays=False),
               dict(out_w=logw), dict(lw=logw, out_w=logw)]  # logw_out without weights, or equal to logw
    for kw in invalid:
        rc, clean = call(**kw)
        assert rc == -1 and clean, kw
    for kw in (dict(V_=(1 << 20) + 1, stride=1 << 21, pmf_stride=1 << 21),):
        rc, clean = call(**kw)
        assert rc == -2 and clean, kw
    for kw in (dict(count=0), dict(batch=0)):  # launch nothing
        rc, clean = call(**kw)
        assert rc == 0 and clean, kw
    assert L.mmt_forecast_scratch_bytes(1, 2 ** 20, 2 ** 11) == -1 and L.mmt_forecast_scratch_bytes(1, 3, 0) == -1
    rc, clean = call(wcount=1, lp=lpm, j0=0, j1=4, lw=logw)
    assert rc == 0 and not clean
