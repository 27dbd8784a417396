"""generate(..., horizon=, realised=) on the fixture of tests/test_gpu_generate_horizon.py (f_small with the given
modalities' heads peaked: prompt 8, 12 new tokens, modalities 1 and 3 generated, 0 and 2 given): a cached run without
num_samples (every row a prompt of one path) and the fan-out engine at S = 16 with evidence="weights" and "resample".

realised= must leave the run alone: sequences, log-probabilities, `ev`, `fc` and `hz` bit-identical to the call without
it. `sc` must equal, bit for bit, the public mmt_sample.horizon_score on the returned sequences, log_weights and `hz`.
A realised series that is one of the returned paths (one with weight) scores a CRPS no larger than the spread of the
paths and a PIT strictly inside (0, 1)."""
import pytest
import torch

import mmt_sample as MS
from test_gpu_generate_evidence import GEN, N, N0, bits, call, inputs
from test_gpu_generate_evidence import peaked_given  # noqa: F401  (a fixture)
from test_gpu_generate_forecast import values_for
from test_gpu_generate_horizon import BARS, PCT

pytestmark = pytest.mark.gpu

KEYS = set(MS.SCORE_FIELDS) | {"pinball", "brier", "agg", "aggq", "aggb", "pit_hist"}


def same_tree(a, b):
    """Bit equality of nested lists / tuples / dicts of tensors (and of plain values)."""
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a) if a.is_floating_point() else a,
                                                                         bits(b) if b.is_floating_point() else b)
    if isinstance(a, dict):
        return sorted(a, key=str) == sorted(b, key=str) and all(same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_tree(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("B,S,evidence", [(3, None, None), (3, 16, "weights"), (3, 16, "resample")])
def test_realised_leaves_the_run_alone_and_is_the_public_score(peaked_given, B, S, evidence):
    meta, idx, m = peaked_given
    start, given = inputs(meta, idx, B)
    vals = values_for(meta)
    kw = dict(num_samples=S, horizon={"values": {i: vals[i] for i in GEN}, "is_percent": {3: True}, "barriers": BARS})
    if evidence is not None:
        kw.update(evidence=evidence)
    if evidence == "resample":
        kw.update(resample_every=3, ess_threshold=2.0)  # every point resamples
    base = call(m, start, given, **kw)
    Sp = S if S is not None else 1
    seqs, hz = base[0], base[-1]
    logw = base[2]["log_weights"] if evidence is not None else None
    # two realised series per modality: a random one, and per prompt the returned path with the largest weight
    g = torch.Generator().manual_seed(7 + B)
    best = (logw.view(B, Sp).argmax(dim=1) if logw is not None else torch.zeros(B, dtype=torch.long, device="cuda"))
    rows = torch.arange(B, device="cuda") * Sp + best
    drawn = {i: torch.randint(0, meta["V"][i], (B, N), generator=g).cuda() for i in GEN}
    member = {i: seqs[i][rows, N0:].long() for i in GEN}
    for name, real in (("drawn", drawn), ("member", member)):
        out = call(m, start, given, realised=real, **kw)
        torch.cuda.synchronize()
        assert len(out) == len(base) + 1 and same_tree(out[:-1], base), name
        sc = out[-1]
        assert sorted(sc) == GEN
        for i in GEN:
            d, nb = sc[i], len(BARS[i])
            assert set(d) == KEYS
            for k in MS.SCORE_FIELDS:
                assert d[k].shape == (B, N) and d[k].dtype == torch.float64, k
            assert d["pinball"].shape == (B, N, 3) and d["brier"].shape == (B, N, nb)
            assert d["agg"].shape == (N, 10) and d["aggq"].shape == (N, 3, 2) and d["aggb"].shape == (N, nb, 3)
            assert d["pit_hist"].shape == (N, 10)
            pub = MS.horizon_score([seqs[i][:, N0:]], [real[i]], samples=Sp, values=[vals[i]], is_percent=PCT[i],
                                   origin=[None if PCT[i] else seqs[i][:, N0 - 1].contiguous()],
                                   realised_origin=[None if PCT[i] else start[i][:, -1].contiguous()], logw=logw,
                                   forecast=[hz[i]], barriers=[BARS[i]])[0]
            assert same_tree(d, pub), (name, i)
            assert bool((d["agg"][:, 0] == B).all()) and bool((d["pit_hist"].sum(dim=1) == B).all())
            assert bool((d["crps"] >= 0).all()) and bool(((d["pit"] >= 0) & (d["pit"] <= 1)).all())
            if name == "member":
                spread = hz[i]["max"] - hz[i]["min"]
                assert bool((d["crps"] <= spread).all()), (i, d["crps"], spread)
                assert bool(((d["pit"] > 0) & (d["pit"] < 1)).all()), (i, d["pit"])
                if Sp == 1:  # the one path is the realised series: a perfect point forecast
                    assert bool((d["crps"] == 0).all()) and bool((d["pit"] == 0.5).all())
                    assert bool((d["mean_error"] == 0).all()) and bool((d["pinball"] == 0).all())
    if evidence == "resample":
        assert base[2]["resampled"].any(), "no prompt was resampled"


def test_realised_refusals_and_one_scored_modality(peaked_given):
    meta, idx, m = peaked_given
    start = [t[:2, :N0].cuda() for t in idx]
    vals = values_for(meta)
    y = torch.zeros(2, 3, dtype=torch.int64, device="cuda")
    hz = {"values": {3: vals[3]}}
    with pytest.raises(ValueError, match="horizon="):
        m.generate(start, max_new_tokens=3, modality_to_generate=GEN, seed=1, realised={3: y})
    with pytest.raises(ValueError, match=r"\[3\]"):
        m.generate(start, max_new_tokens=3, modality_to_generate=3, seed=1, realised={3: y})
    for bad in ({1: y}, {0: y}, {3: y.int()}, {3: y[:, :2]}, {3: y[:1]}, {}, [y]):
        with pytest.raises(ValueError):
            m.generate(start, max_new_tokens=3, modality_to_generate=GEN, seed=1, horizon=hz, realised=bad)
    # one modality scored, no barriers, no forecast=: `sc` follows `hz`; a token outside the vocabulary kills its prompt
    y[1, 2] = meta["V"][3]
    seqs, h, sc = m.generate(start, max_new_tokens=3, modality_to_generate=GEN, seed=1, horizon=hz, realised={3: y})
    assert sorted(sc) == [3] and sc[3]["brier"].shape == (2, 3, 0) and sc[3]["aggb"].shape == (3, 0, 3)
    assert bool(torch.isnan(sc[3]["crps"][1]).all()) and bool(torch.isfinite(sc[3]["crps"][0]).all())
    assert sc[3]["agg"][:, 0].tolist() == [1.0] * 3
    v = torch.as_tensor(vals[3], dtype=torch.float64)
    x0 = v[0] - v[start[3][0, -1].cpu()]  # a value series: the change of the realised tokens (all 0) from the prompt's last
    assert sc[3]["realised"][0].cpu().tolist() == [float(x0)] * 3
    out = m.generate(start, max_new_tokens=2, modality_to_generate=GEN, seed=1, horizon=hz, realised=None)
    assert isinstance(out, tuple) and len(out) == 2
