"""generate(..., horizon=) on the fixture and helpers of tests/test_gpu_generate_evidence.py (f_small with the given
modalities' heads peaked: prompt 8, 12 new tokens, modalities 1 and 3 generated, 0 and 2 given): a cached run without
num_samples (every row a prompt of one path) and the fan-out engine at S = 16 with evidence="weights" and "resample".

horizon= must leave the run alone: sequences, log-probabilities, `ev` and `fc` bit-identical to the call without it.
`hz` must equal, bit for bit, the public mmt_sample.horizon_stats on the returned sequences and log_weights, and agree
with tests/horizon_ref.py under the bounds of tests/test_gpu_horizon.py."""
import numpy as np
import pytest
import torch

import horizon_ref as H
import mmt_sample as MS
from test_gpu_generate_evidence import GEN, N, N0, bits, call, inputs
from test_gpu_generate_evidence import peaked_given  # noqa: F401  (a fixture)
from test_gpu_generate_forecast import values_for

pytestmark = pytest.mark.gpu

QUANT = [0.1, 0.5, 0.9]
BARS = {1: [1.0, -1.0], 3: [0.5, -0.5, 2.0]}  # of unequal lengths: one call pads the shorter list
PCT = {1: False, 3: True}
KEYS = set(MS.HORIZON_FIELDS) | {"quantile_values", "quantile_paths", "hit", "ess", "live"}


def as_numpy(d):
    stats = torch.stack([d[k] for k in MS.HORIZON_FIELDS], dim=-1).cpu().numpy()
    return {"stats": stats, "qval": d["quantile_values"].cpu().numpy(), "qrow": d["quantile_paths"].cpu().numpy(),
            "hit": d["hit"].cpu().numpy(), "ess": d["ess"].cpu().numpy(), "live": d["live"].cpu().numpy()}


@pytest.mark.parametrize("B,S,evidence", [(3, None, None), (3, 16, "weights"), (3, 16, "resample")])
def test_horizon_leaves_the_run_alone_and_follows_the_rule(peaked_given, B, S, evidence):
    meta, idx, m = peaked_given
    start, given = inputs(meta, idx, B)
    vals = values_for(meta)
    kw = dict(num_samples=S, forecast={"quantiles": QUANT, "values": vals, "is_percent": {3: True}})
    if evidence is not None:
        kw.update(evidence=evidence)
    if evidence == "resample":
        kw.update(resample_every=3, ess_threshold=2.0)  # every point resamples
    base = call(m, start, given, **kw)
    out = call(m, start, given, horizon={"barriers": BARS}, **kw)  # values and is_percent come from forecast=
    torch.cuda.synchronize()
    assert len(out) == len(base) + 1
    assert all(torch.equal(a, b) for a, b in zip(out[0], base[0]))
    assert all(torch.equal(bits(out[1][i]), bits(base[1][i])) for i in GEN)
    if evidence is not None:
        ev, ev0 = out[2], base[2]
        for k in ("log_weights", "log_evidence", "ancestors", "resampled"):
            assert torch.equal(bits(ev[k]), bits(ev0[k])), k
        assert all(torch.equal(bits(ev["given_logprobs"][i]), bits(ev0["given_logprobs"][i])) for i in ev0["given_logprobs"])
    fc, fc0 = out[-2], base[-1]
    assert all(torch.equal(bits(fc[i][k]), bits(fc0[i][k])) for i in GEN for k in fc0[i])

    hz = out[-1]
    Sp, Bp = (S, B) if S is not None else (1, B)
    assert sorted(hz) == GEN
    seqs = out[0]
    logw = out[2]["log_weights"] if evidence is not None else None
    for i in GEN:
        d = hz[i]
        nb = len(BARS[i])
        assert set(d) == KEYS
        for k in MS.HORIZON_FIELDS:
            assert d[k].shape == (Bp, N) and d[k].dtype == torch.float64, k
        assert d["quantile_values"].shape == (Bp, N, 3) and d["quantile_values"].dtype == torch.float64
        assert d["quantile_paths"].shape == (Bp, N, 3) and d["quantile_paths"].dtype == torch.int32
        assert d["hit"].shape == (Bp, N, nb) and d["ess"].shape == (Bp,) and d["live"].dtype == torch.int32
        # the public wrapper on what generate returned (the default quantiles of horizon= are not forecast='s)
        pub = MS.horizon_stats([seqs[i][:, N0:]], samples=Sp, values=[vals[i]], is_percent=PCT[i],
                               origin=[None if PCT[i] else seqs[i][:, N0 - 1].contiguous()], logw=logw,
                               barriers=[BARS[i]])[0]
        got, want = as_numpy(d), as_numpy(pub)
        for k in got:
            a, b = got[k], want[k]
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                  b.view(np.int64) if b.dtype == np.float64 else b), (i, k)
        # the rule
        tok = seqs[i][:, N0:].cpu().numpy()
        pq = H.paths(tok, vals[i], PCT[i], seqs[i][:, N0 - 1].cpu().numpy())
        a = None if logw is None else logw.cpu().numpy()
        worst = amb = 0
        for b in range(Bp):
            sl = slice(b * Sp, (b + 1) * Sp)
            ref = H.prompt(*[t[sl] for t in pq], None if a is None else a[sl], H.LEVELS, BARS[i])
            n_amb, w = H.check({k: v[b] for k, v in got.items()}, ref, a is not None, f"modality {i} prompt {b}")
            worst, amb = max(worst, w), amb + n_amb
            if Sp == 1:  # one path: every quantile is the path's own x, a barrier is touched or not
                x = pq[0][b]
                assert np.array_equal(got["qval"][b], np.repeat(x[:, None], 3, axis=1)) and (got["qrow"][b] == 0).all()
                assert np.isin(got["hit"][b], (0.0, 1.0)).all() and got["ess"][b] == 1.0 and got["live"][b] == 1
                assert np.array_equal(got["stats"][b][:, 0], x) and (got["stats"][b][:, 1] == 0).all()
        assert amb <= H.cap(Bp * N * 3)
        assert (np.diff(got["hit"], axis=1) >= 0).all()
        print(f"generate horizon B={B} S={S} evidence={evidence} modality {i}: max error / bound {worst:.3f}, "
              f"ambiguous {amb}")
    if evidence == "resample":
        assert out[2]["resampled"].any(), "no prompt was resampled"


def test_horizon_refusals_and_own_values(peaked_given):
    meta, idx, m = peaked_given
    start = [t[:2, :N0].cuda() for t in idx]
    vals = values_for(meta)
    with pytest.raises(ValueError, match=r"\[1\]"):
        m.generate(start, max_new_tokens=2, modality_to_generate=1, seed=1, horizon={"values": {1: vals[1]}})
    for bad in (True, {"values": {0: np.zeros(meta["V"][0])}}, {"values": {1: vals[1]}, "barriers": {1: [0.0]}},
                {"values": {1: vals[1]}, "barriers": {1: [1.0] * 9}}, {"values": {1: vals[1]}, "levels": [0.5]}):
        with pytest.raises(ValueError):
            m.generate(start, max_new_tokens=2, modality_to_generate=GEN, seed=1, horizon=bad)
    with pytest.raises(ValueError, match="4096"):
        m.generate(start, max_new_tokens=2, modality_to_generate=GEN, seed=1, num_samples=4097,
                   horizon={"values": {1: vals[1]}})
    # its own values, one modality reported, no forecast=, no barriers: `hz` is the last element after the sequences
    seqs, hz = m.generate(start, max_new_tokens=3, modality_to_generate=GEN, seed=1, horizon={"values": {3: vals[3]}})
    assert sorted(hz) == [3] and hz[3]["hit"].shape == (2, 3, 0) and hz[3]["mean"].shape == (2, 3)
    x = H.paths(seqs[3][:, N0:].cpu().numpy(), vals[3], False, seqs[3][:, N0 - 1].cpu().numpy())[0]
    assert np.array_equal(hz[3]["mean"].cpu().numpy(), x)
    out = m.generate(start, max_new_tokens=2, modality_to_generate=GEN, seed=1, horizon=False)
    assert isinstance(out, list) and len(out) == len(start)
