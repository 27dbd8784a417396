"""generate(num_samples=S, rolling=True) end to end on the GPU: rollouts that start from a full context window.

The model recipe is test_gpu_decode_fanout.py's (3 modalities, cross-attention on modality 0, the repository oracle).
Logits a cloning logits_hook captured at every sequence length n are re-sampled with mmt_sample.sample (tokens and
log-probabilities bit for bit: draws keyed by (seed, row, position)) and compared with the full forward over each
path's own block_size window, model([s[:, n - T:n] for s in seqs]) at the last position, and with the oracle on the same
window, under the three criteria of test_gpu_decode_fanout.py.
"""
import pytest
import torch

import config_utils
import mmt_sample as MS
from golden_io import model_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
V3, CROSS3 = [37, 5, 11], [True, False, False]
FACTOR = 2.0
T, B, S = 24, 2, 3


def rel(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def build(meta, sd, dropout=0.0):
    config_utils._config_cache = {"n_embd": meta["n_embd"], "n_head": meta["n_head"], "n_layer": meta["n_layer"],
                                  "block_size": meta["block_size"], "dropout": dropout, "device": "cuda",
                                  "batch_size": meta["B"], "eval_iters": 1}
    import model as mmt_model
    params = []
    for i, v in enumerate(meta["V"]):
        p = [None] * 12
        p[8] = meta["cross"][i]
        params.append(p)
    m = mmt_model.MultimodalTransformer(len(meta["V"]), meta["V"], params).to("cuda")
    full = dict(sd)
    Tb = meta["block_size"]
    for k in meta["state_dict_keys"]:
        if k.endswith("tril"):
            full[k] = torch.tril(torch.ones(Tb, Tb))
    m.load_state_dict(full, strict=True)
    return m


def _model(hs, H, L, Tb, Bm, seed):
    import mmt_oracle as O
    C = H * hs
    cfg = O.OracleConfig(C, H, L, Tb, V3, CROSS3)
    g = torch.Generator().manual_seed(seed)
    sd = O.init_params(cfg, g)
    for k in sd:
        if k.endswith("bias") or "ln" in k or "norm" in k:
            sd[k] = sd[k] + 0.05 * torch.randn(sd[k].shape, generator=g)
    tril = [f"blocks.{l}.{kind}.{i}.heads.{h}.tril" for l in range(L) for i in range(len(V3))
            for kind in ("sa_layers", "cross_attention_layers") for h in range(H)
            if kind == "sa_layers" or CROSS3[i]]
    meta = {"n_embd": C, "n_head": H, "n_layer": L, "block_size": Tb, "B": Bm, "V": V3, "cross": CROSS3,
            "state_dict_keys": list(sd.keys()) + tril}
    m = build(meta, sd)
    m.eval()
    idx = [torch.randint(0, v, (Bm, Tb), generator=g) for v in V3]
    return m, sd, cfg, idx, g


@pytest.fixture(scope="module")
def small():
    return _model(32, 2, 2, T, B, seed=77)


def _windows(m, sd, cfg, seqs, lengths, gmod):
    """Per sequence length n: the full forward's and the oracle's logits of modality gmod at the last position of
    each path's window s[:, n - T:n] (n >= T), or of the padded sequence at position n - 1 (n < T); and e_full, the
    full forward's own worst per-position deviation from the oracle over everything it ran."""
    import mmt_oracle as O
    full_last, ref_last, e_full = {}, {}, 0.0
    for n in lengths:
        lo = max(0, n - T)
        win = [s[:, lo:n] for s in seqs]
        with torch.no_grad():
            full, _ = m(win)
        f = full[gmod].cpu()
        ref, _ = O.forward(sd, cfg, [torch.nn.functional.pad(w.cpu(), (0, T - (n - lo))) for w in win])
        r = ref[gmod][:, :n - lo]
        e_full = max(e_full, max(rel(f[:, t], r[:, t]) for t in range(n - lo)))
        full_last[n], ref_last[n] = f[:, -1], r[:, -1]
    return full_last, ref_last, e_full


def _criteria(what, seen, full_last, ref_last, e_full, lengths):
    got = torch.stack([seen[n].cpu() for n in lengths], dim=1)
    fg = torch.stack([full_last[n] for n in lengths], dim=1)
    rg = torch.stack([ref_last[n] for n in lengths], dim=1)
    per = [rel(seen[n], ref_last[n]) for n in lengths]
    print(f"generate rolling, {what}: stacked rel vs full {rel(got, fg):.2e}, vs oracle {rel(got, rg):.2e}, per position "
          f"max {max(per):.2e}, e_full {e_full:.2e}, ratio {max(per) / e_full:.2f}")
    assert rel(got, fg) < 1e-2, what
    assert rel(got, rg) < 2e-2, what
    assert max(per) <= FACTOR * e_full, (what, per, e_full)


def _resampled(seen, seqs, lp, n0, N, gmod, seed, **settings):
    for n in range(n0, n0 + N):
        tok, l = MS.sample(seen[n], seed=seed, row0=0, pos=n, return_logprobs=True, **settings)
        assert torch.equal(tok, seqs[gmod][:, n]), n
        assert torch.equal(l, lp[:, n - n0]), n


def test_generate_from_a_full_window(small):
    m, sd, cfg, idx, g = small
    n0, N, gmod, seed = T, 6, 0, 1234
    prompts = [t[:, :n0].cuda() for t in idx]
    seen = {}
    hook = lambda n, lg: seen.__setitem__(n, lg.clone())  # noqa: E731
    kw = dict(max_new_tokens=N, modality_to_generate=gmod, temperature=0.9, top_k=5, seed=seed, return_logprobs=True)
    seqs, lp = m.generate(prompts, logits_hook=hook, num_samples=S, rolling=True, **kw)
    assert m.last_generate_path == "rolling"
    R = B * S
    assert all(tuple(s.shape) == (R, n0 + N) for s in seqs) and tuple(lp.shape) == (R, N)
    assert sorted(seen) == list(range(n0, n0 + N)) and all(tuple(v.shape) == (R, V3[gmod]) for v in seen.values())
    for i in range(len(V3)):  # the prompts, tiled, and the other modalities' pad with their last token
        assert torch.equal(seqs[i][:, :n0], prompts[i].repeat_interleave(S, 0))
        if i != gmod:
            assert (seqs[i][:, n0:] == seqs[i][:, n0 - 1:n0]).all()
    _resampled(seen, seqs, lp, n0, N, gmod, seed, temperature=0.9, top_k=5)
    lengths = list(range(n0, n0 + N))
    _criteria("full window", seen, *_windows(m, sd, cfg, seqs, lengths, gmod), lengths)
    # the same call again: the same bits (the rolling step keeps no state)
    seqs2, lp2 = m.generate(prompts, num_samples=S, rolling=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(seqs, seqs2)) and torch.equal(lp, lp2)
    # without the keyword the call is tiled, as before
    seqs3, lp3 = m.generate(prompts, num_samples=S, **kw)
    assert m.last_generate_path == "tiled" and all(tuple(s.shape) == (R, n0 + N) for s in seqs3)


def test_generate_mixed_existing_steps_then_rolling(small):
    """n0 = T - 2, N = 6: the prefill and the two fan-out steps that still fit the block are the existing engine's,
    bit for bit; the three steps past it roll."""
    m, sd, cfg, idx, g = small
    n0, N, gmod, seed = T - 2, 6, 0, 99
    prompts = [t[:, :n0].cuda() for t in idx]
    seen = {}
    hook = lambda n, lg: seen.__setitem__(n, lg.clone())  # noqa: E731
    kw = dict(modality_to_generate=gmod, temperature=0.8, seed=seed, return_logprobs=True)
    seqs, lp = m.generate(prompts, max_new_tokens=N, logits_hook=hook, num_samples=S, rolling=True, **kw)
    assert m.last_generate_path == "rolling"
    _resampled(seen, seqs, lp, n0, N, gmod, seed, temperature=0.8)
    # steps 0 and 1 against the call of N = 2 without the keyword (the fan-out engine) ...
    seen2 = {}
    a, la = m.generate(prompts, max_new_tokens=2, logits_hook=lambda n, lg: seen2.__setitem__(n, lg.clone()),
                       num_samples=S, **kw)
    assert m.last_generate_path == "fanout"
    assert all(torch.equal(x[:, :n0 + 2], y) for x, y in zip(seqs, a)) and torch.equal(lp[:, :2], la)
    assert torch.equal(seen[n0], seen2[n0]) and torch.equal(seen[n0 + 1], seen2[n0 + 1])
    # ... and steps 1 and 2 against the fan-out engine's own steps at positions T - 2 and T - 1 (a call of N = 3
    # without the keyword is tiled: n0 + 3 > T)
    with torch.no_grad():
        m(prompts)
        for pos in (n0, n0 + 1):
            step = m._decode_fanout_step([s[:, pos] for s in seqs], pos, S, n0, T - n0)
            assert torch.equal(step[gmod], seen[pos + 1]), pos
    m.generate(prompts, max_new_tokens=3, num_samples=S, **kw)
    assert m.last_generate_path == "tiled"
    lengths = list(range(T + 1, n0 + N))
    assert len(lengths) == 3
    _criteria("mixed", seen, *_windows(m, sd, cfg, seqs, lengths, gmod), lengths)


def test_generate_greedy_rolling_equals_tiled():
    """Peaked output heads (the x60 recipe of test_generate_greedy_fanout_equals_tiled), temperature 0, n0 = T: the
    rolling tokens equal the tiled call's, and all samples of a prompt coincide."""
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    sd = dict(sd)
    for k in list(sd):
        if k.startswith("post_block.soft_score_layers.") and k.endswith(".2.weight"):
            sd[k] = sd[k] * 60.0
    m = build(meta, sd)
    m.eval()
    Tb, Sg, N = meta["block_size"], 5, 5
    start = [t[:2, :Tb].cuda() for t in idx]
    a = m.generate(start, max_new_tokens=N, modality_to_generate=2, temperature=0, num_samples=Sg, rolling=True)
    assert m.last_generate_path == "rolling"
    b = m.generate(start, max_new_tokens=N, modality_to_generate=2, temperature=0, num_samples=Sg)
    assert m.last_generate_path == "tiled"
    for i in range(cfg.M):
        assert tuple(a[i].shape) == (2 * Sg, Tb + N) and torch.equal(a[i], b[i]), i
        assert torch.equal(a[i][0::Sg].repeat_interleave(Sg, 0), a[i]), i


def test_generate_rolling_equivalences_and_fallbacks(small):
    m, sd, cfg, idx, g = small
    kw = dict(modality_to_generate=0, temperature=0.8, seed=9, return_logprobs=True, num_samples=S)
    inside = [t[:, :5].cuda() for t in idx]
    # inside the block: the fan-out engine, bit for bit the call without the keyword
    a, la = m.generate(inside, max_new_tokens=T - 5, rolling=True, **kw)
    assert m.last_generate_path == "fanout"
    b, lb = m.generate(inside, max_new_tokens=T - 5, **kw)
    assert m.last_generate_path == "fanout"
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(la, lb)
    # the last step reads exactly T tokens: no rolling step would run, tiled as without the keyword
    c, lc = m.generate(inside, max_new_tokens=T - 4, rolling=True, **kw)
    assert m.last_generate_path == "tiled"
    d, ld = m.generate(inside, max_new_tokens=T - 4, **kw)
    assert all(torch.equal(x, y) for x, y in zip(c, d)) and torch.equal(lc, ld)
    full = [t[:, :T].cuda() for t in idx]
    m.generate(full, max_new_tokens=3, use_cache=False, rolling=True, **kw)
    assert m.last_generate_path == "tiled"
    e, le = m.generate(full, max_new_tokens=T + 1, rolling=True, **kw)  # N > T: the prefix would run out of rows
    assert m.last_generate_path == "tiled" and tuple(le.shape) == (B * S, T + 1)
    e2, le2 = m.generate(full, max_new_tokens=T, rolling=True, **kw)  # N = T: the last step shares one row
    assert m.last_generate_path == "rolling" and tuple(le2.shape) == (B * S, T)
    assert torch.isfinite(le2).all()
    with pytest.raises(ValueError, match="num_samples"):
        m.generate(full, max_new_tokens=3, modality_to_generate=0, seed=1, rolling=True)


def _pmf_of(views, mods, settings, **kw):
    pmfs, ess, live = MS.forecast_multi([views[i] for i in mods], samples=S, temperature=[settings[i][0] for i in mods],
                                        top_k=[settings[i][1] for i in mods], top_p=[settings[i][2] for i in mods], **kw)
    return pmfs


def test_generate_rolling_list_form_forecast_horizon_evidence(small):
    """The list form on rolling steps. "all" with forecast= and horizon=: the pmf of step j is
    mmt_sample.forecast_multi over the views the hook captured. evidence= needs a given modality, which "all" leaves
    none for, so evidence="weights" runs on [0, 2] with modality 1 given: its pmf is forecast_multi's under the
    returned scores of the given columns 0..j. evidence="resample" across the block raises."""
    m, sd, cfg, idx, g = small
    n0, N, seed = T, 5, 31
    prompts = [t[:, :n0].cuda() for t in idx]
    settings = {0: (0.9, 5, 1.0), 1: (1.0, 0, 1.0), 2: (0.7, 0, 0.9)}
    vals = {0: torch.linspace(-2.0, 2.0, V3[0], dtype=torch.float64)}
    seen = {}
    hook = lambda n, views: seen.__setitem__(n, [v.clone() for v in views])  # noqa: E731
    kw = dict(max_new_tokens=N, temperature={i: s[0] for i, s in settings.items()}, seed=seed, num_samples=S, rolling=True,
              top_k={0: 5}, top_p={2: 0.9})
    seqs, fc, hz = m.generate(prompts, modality_to_generate="all", forecast=True,
                              horizon={"values": vals, "barriers": {0: [1.0]}}, logits_hook=hook, **kw)
    assert m.last_generate_path == "rolling"
    base = m.generate(prompts, modality_to_generate="all", **kw)
    assert all(torch.equal(x, y) for x, y in zip(seqs, base))
    assert sorted(fc) == [0, 1, 2] and sorted(hz) == [0]
    assert tuple(hz[0]["mean"].shape) == (B, N) and torch.isfinite(hz[0]["mean"]).all()
    for j in range(N):
        pm = _pmf_of(seen[n0 + j], [0, 1, 2], settings)
        for p, i in enumerate((0, 1, 2)):
            assert torch.equal(fc[i]["pmf"][:, j], pm[p]), (i, j)
    # with a given modality and its evidence
    gen = [0, 2]
    given = {1: torch.randint(0, V3[1], (B, N), generator=g)}
    seen.clear()
    kw2 = dict(kw, temperature={0: 0.9, 2: 0.7})
    seqs, ev, fc, hz = m.generate(prompts, modality_to_generate=gen, given=given, evidence="weights", forecast=True,
                                  horizon={"values": vals}, logits_hook=hook, **kw2)
    assert m.last_generate_path == "rolling"
    assert torch.equal(seqs[1][:, n0:], given[1].cuda().repeat_interleave(S, 0))
    glp = ev["given_logprobs"][1]
    for j in range(N):
        pm = _pmf_of(seen[n0 + j], gen, settings, logprobs=[glp], j0=0, j1=j + 1)
        for p, i in enumerate(gen):
            assert torch.equal(fc[i]["pmf"][:, j], pm[p]), (i, j)
    assert torch.isfinite(ev["log_evidence"]).all() and tuple(hz[0]["mean"].shape) == (B, N)
    with pytest.raises(ValueError, match="resample"):
        m.generate(prompts, modality_to_generate=gen, given=given, evidence="resample", **kw2)
