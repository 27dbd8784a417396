"""generate(..., forecast=) on the fixture and helpers of tests/test_gpu_generate_evidence.py (f_small with the given
modalities' heads peaked: prompt 8, 12 new tokens, modalities 1 and 3 generated with temperature 0.9 / top-k 3,
modalities 0 and 2 given): the fan-out engine, tiled re-forwards (use_cache=False) and no num_samples, each without
evidence, with evidence="weights" and, on the fan-out engine, evidence="resample".

forecast= must leave the run alone: sequences, log-probabilities and `ev` bit-identical to the call without it. The
returned pmf is compared with tests/forecast_ref.py applied to the logits a cloning logits_hook saw and to the
device's scores of the given tokens (the hook scores them with the public score_multi, the kernel generate runs, as
the evidence test does), within the bound of tests/test_gpu_forecast.py. The weights of step j are replayed from
those scores: the carried log-weights (reset where `ev` says a prompt was resampled) plus the columns since the last
resampling point through j."""
import numpy as np
import pytest
import torch

import evidence_ref as E
import forecast_ref as F
from test_gpu_generate_evidence import GEN, GIVEN, N, N0, SETTINGS, Recorder, bits, call, inputs
from test_gpu_generate_evidence import peaked_given  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

QUANT = [0.1, 0.5, 0.9]
KEYS = {"pmf", "ess", "live", "entropy", "mean", "var", "p_down", "p_flat", "p_up", "quantile_tokens",
        "quantile_values"}


def values_for(meta):
    return {1: np.linspace(-1.0, 5.0, meta["V"][1]), 3: np.array([-2.0, -0.5, 0.0, 0.0, 1.0])}


@pytest.mark.parametrize("B,S,use_cache,evidence", [
    (3, 17, True, None), (3, 17, True, "weights"), (3, 17, True, "resample"), (1, 8, True, "resample"),
    (3, 17, False, None), (3, 17, False, "weights"), (3, None, True, None), (3, None, True, "weights")])
def test_forecast_leaves_the_run_alone_and_follows_the_rule(peaked_given, B, S, use_cache, evidence):
    meta, idx, m = peaked_given
    start, given = inputs(meta, idx, B)
    kw = dict(num_samples=S, use_cache=use_cache)
    if evidence is not None:
        kw.update(evidence=evidence)
    if evidence == "resample":
        kw.update(resample_every=3, ess_threshold=2.0)  # every point resamples
    base = call(m, start, given, **kw)
    vals = values_for(meta)
    rec = Recorder(given, S)
    out = call(m, start, given, logits_hook=rec,
               forecast={"quantiles": QUANT, "values": vals, "is_percent": {3: True}}, **kw)
    torch.cuda.synchronize()
    if S is not None:
        assert m.last_generate_path == ("fanout" if use_cache else "tiled")
    fc = out[-1]
    assert len(out) == len(base) + 1
    assert all(torch.equal(a, b) for a, b in zip(out[0], base[0]))
    assert all(torch.equal(bits(out[1][i]), bits(base[1][i])) for i in GEN)
    if evidence is not None:
        ev, ev0 = out[2], base[2]
        assert all(torch.equal(bits(ev["given_logprobs"][i]), bits(ev0["given_logprobs"][i])) for i in GIVEN)
        for k in ("log_weights", "log_evidence", "ancestors", "resampled"):
            assert torch.equal(bits(ev[k]), bits(ev0[k])), k
        assert ev["steps"] == ev0["steps"]

    Sp = S or 1
    rows, Bp = B * Sp, B if S is not None else B
    assert sorted(fc) == GEN
    resampled = out[2]["resampled"].cpu().numpy() if evidence == "resample" else None
    steps = out[2]["steps"] if evidence is not None else []
    worst = 0.0
    for i in GEN:
        f = fc[i]
        V = meta["V"][i]
        assert set(f) == KEYS
        assert f["pmf"].shape == (Bp, N, V) and f["pmf"].dtype == torch.float32
        assert f["ess"].shape == (Bp, N) and f["ess"].dtype == torch.float64
        assert f["live"].shape == (Bp, N) and f["live"].dtype == torch.int32
        for k in ("entropy", "mean", "var", "p_down", "p_flat", "p_up"):
            assert f[k].shape == (Bp, N) and f[k].dtype == torch.float64, k
        assert f["quantile_tokens"].shape == (Bp, N, 3) and f["quantile_tokens"].dtype == torch.int32
        assert f["quantile_values"].shape == (Bp, N, 3) and f["quantile_values"].dtype == torch.float64
        pmf, ess, live = f["pmf"].cpu().numpy(), f["ess"].cpu().numpy(), f["live"].cpu().numpy()
        logw, since = np.zeros(rows), 0
        for j in range(N):
            laws = F.row_laws(rec.logits[N0 + j][i].cpu().numpy(), *SETTINGS[i])
            a = None
            if evidence is not None:
                cols = [np.stack([rec.glp[jj][p] for jj in range(since, j + 1)], axis=1) for p in range(len(GIVEN))]
                a = E.accumulate(logw, cols, 0, j + 1 - since)
            for b in range(Bp):
                sl = slice(b * Sp, (b + 1) * Sp)
                ref = F.mixture(laws, np.arange(rows)[sl], None if a is None else a[sl])
                ratio, bad = F.check_pmf(pmf[b, j], ref)
                worst = max(worst, ratio)
                assert not bad, (i, j, b, ratio)
                assert int(live[b, j]) == ref["live"] == Sp
                assert abs(ess[b, j] - ref["ess"]) <= 4 * F.EPS_W * ref["ess"]
            if j in steps:  # a resampling point: a resampled prompt restarts at weight 1, the others carry a_s
                pt = steps.index(j)
                for b in range(Bp):
                    sl = slice(b * Sp, (b + 1) * Sp)
                    logw[sl] = 0.0 if resampled[pt, b] else a[sl]
                since = j + 1
        # the summaries are functions of the stored pmf: the restatement on the device's rows
        st = {k: f[k].cpu().numpy() for k in KEYS - {"pmf", "ess", "live"}}
        origin = start[i][:, -1].cpu().numpy()
        for b in range(Bp):
            for j in range(N):
                want, qt, alt = F.pmf_stats(pmf[b, j], vals[i], i == 3, origin[b], QUANT)
                got = np.array([st[k][b, j] for k in ("entropy", "mean", "var", "p_down", "p_flat", "p_up")])
                assert np.all(np.abs(got - want[1:7]) <= 1e-12 * np.abs(want[1:7])), (i, b, j, got, want)
                g = st["quantile_tokens"][b, j]
                assert np.all((g == qt) | (g == alt))
                assert np.array_equal(st["quantile_values"][b, j], vals[i][g])
    if evidence == "resample":
        assert resampled.any(), "no prompt was resampled: the replay of the weights was not exercised"
    print(f"generate forecast B={B} S={S} cache={use_cache} evidence={evidence}: max error / bound {worst:.3f}")


def test_step_zero_is_the_reference_certainty_rule(peaked_given):
    """At temperature 1 without top-k / top-p, step 0's p_up / p_flat / p_down are the reference's directional
    certainty on the prefill logits: the softmax mass of the tokens whose _get_direction_sign against the last prompt
    token (a value series) or whose own sign (a percent series) is +1 / 0 / -1. Tolerance: twice the summed
    per-element bound of the pmf (its fp32 rounding and the normaliser), plus the stored row's T - 1."""
    meta, idx, m = peaked_given
    B = 3
    start = [t[:B, :N0].cuda() for t in idx]
    vals = values_for(meta)
    seen = {}

    def hook(n, views):
        if n == N0:
            seen.update({i: views[i].clone() for i in GEN})

    seqs, fc = m.generate(start, max_new_tokens=2, modality_to_generate=GEN, seed=5, logits_hook=hook,
                          forecast={"values": vals, "is_percent": {3: True}})
    for i in GEN:
        logits = seen[i].cpu().numpy()
        probs = torch.softmax(seen[i].double(), dim=-1).cpu().numpy()
        laws = F.row_laws(logits, 1.0, 0, 1.0)
        for b in range(B):
            vo = vals[i][int(start[i][b, -1])]
            sign = np.array([F.direction_sign(float(v), vo, i == 3) for v in vals[i]])
            tol = 2 * F.mixture(laws, [b])["bound"].sum() + 2.0 ** -20
            for key, sg in (("p_down", -1), ("p_flat", 0), ("p_up", 1)):
                want = probs[b][sign == sg].sum()
                assert abs(float(fc[i][key][b, 0]) - want) <= tol, (i, b, key)
            assert abs(float(fc[i]["p_down"][b, 0] + fc[i]["p_flat"][b, 0] + fc[i]["p_up"][b, 0]) - 1) <= 1e-12
    assert fc[3]["quantile_tokens"].shape == (B, 2, 3)  # the default levels


def test_forecast_refusals(peaked_given):
    meta, idx, m = peaked_given
    start = [t[:2, :N0].cuda() for t in idx]
    with pytest.raises(ValueError, match=r"\[1\]"):
        m.generate(start, max_new_tokens=2, modality_to_generate=1, seed=1, forecast=True)
    for bad in ({"values": {1: np.linspace(5.0, -1.0, meta["V"][1])}}, {"quantiles": [0.5, 1.0]}, {"quantiles": [0.0]},
                {"values": {0: np.zeros(meta["V"][0])}}, {"values": {1: np.zeros(3)}}, {"levels": [0.5]}, 3):
        with pytest.raises(ValueError):
            m.generate(start, max_new_tokens=2, modality_to_generate=GEN, seed=1, forecast=bad)
    out = m.generate(start, max_new_tokens=2, modality_to_generate=GEN, seed=1, forecast=False)
    assert isinstance(out, list) and len(out) == len(start)  # off: the return value of the call without it
