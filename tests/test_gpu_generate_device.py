"""generate's device path (temperature / top_k / top_p / seed / return_logprobs / logits_hook: mmt_rollout.py
rollout_int over mmt_sample_multi) on the f_small fixture (d64, T32, B4, V = [57, 13, 24, 5], cross-attention).

Tokens and log-probabilities are compared with the CPU restatement of the rule (tests/sampling_ref.py) on exactly
the logits the sampler read (logits_hook), under the clear / ambiguous rule and the delta and log-probability bounds
derived in tests/test_gpu_sample.py."""
import numpy as np
import pytest
import torch

import config_utils
import sampling_ref as R
from golden_io import model_fixture
from test_gpu_sample import delta, lp_tol

pytestmark = pytest.mark.gpu


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
    T = meta["block_size"]
    for k in meta["state_dict_keys"]:
        if k.endswith("tril"):
            full[k] = torch.tril(torch.ones(T, T))
    m.load_state_dict(full, strict=True)
    m.eval()
    return m


@pytest.fixture(scope="module")
def small():
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    return meta, cfg, sd, idx, build(meta, sd)


@pytest.fixture(scope="module")
def peaked():
    """f_small with peaked output heads (argmax stable to bf16 noise), as test_generate_kv_cache_greedy_matches_reforward."""
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    sd = dict(sd)
    for k in list(sd):
        if k.startswith("post_block.soft_score_layers.") and k.endswith(".2.weight"):
            sd[k] = sd[k] * 60.0
    return meta, cfg, idx, build(meta, sd)


def test_generate_reproduces_the_rule_on_its_own_logits(small):
    """Prompt of 5, T + 3 - 5 new tokens: the first step samples from the prefill's logits (read in place at the
    last position), the next ones from decode steps, the last three from re-forwards past block_size."""
    meta, cfg, sd, idx, m = small
    T, g, seed = meta["block_size"], 0, 0xC0FFEE1234
    V = meta["V"][g]
    start = [t[:, :5].cuda() for t in idx]
    n_new = T + 3 - 5
    seen = []

    def hook(n, logits):
        assert tuple(logits.shape) == (start[0].shape[0], V) and logits.dtype == torch.float32
        seen.append((n, logits.clone()))

    seqs, lps = m.generate(start, max_new_tokens=n_new, modality_to_generate=g, temperature=0.8, top_k=5, top_p=0.9,
                           seed=seed, return_logprobs=True, logits_hook=hook)
    torch.cuda.synchronize()
    assert [n for n, _ in seen] == list(range(5, 5 + n_new))
    assert tuple(lps.shape) == (start[0].shape[0], n_new) and lps.dtype == torch.float32
    out, lps = seqs[g].cpu().numpy(), lps.cpu().numpy().astype(np.float64)
    d, amb_total = delta(V), 0
    for j, (n, lg) in enumerate(seen):
        ref = R.sample_rows(lg.cpu().numpy(), 0.8, 5, 0.9, seed, n, 0)
        amb, bad = R.check_tokens(ref, out[:, n], d)
        assert not bad, (n, bad, out[:, n], ref["token"], ref["neighbor"])
        amb_total += amb
        clear = (ref["margin_u"] >= d) & (ref["margin_p"] >= d)
        err = np.abs(lps[:, j] - ref["logprob"])[clear]
        assert np.all(err <= lp_tol(V, ref["logprob"][clear])), (n, err)
    print(f"ambiguous rows {amb_total}/{out.shape[0] * n_new}")
    assert amb_total <= 0.05 * out.shape[0] * n_new


def test_generate_same_call_twice_and_across_cache_modes_of_one_seed(small):
    meta, cfg, sd, idx, m = small
    start = [t[:, :7].cuda() for t in idx]
    kw = dict(max_new_tokens=12, modality_to_generate=2, temperature=1.1, top_k=6, seed=99, return_logprobs=True)
    a, la = m.generate(start, **kw)
    b, lb = m.generate(start, **kw)
    for i in range(cfg.M):
        assert torch.equal(a[i], b[i]), i
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    c, _ = m.generate(start, **dict(kw, seed=100))
    assert not torch.equal(a[2], c[2])


def test_generate_greedy_cache_equals_reforward_equals_argmax_path(peaked):
    meta, cfg, idx, m = peaked
    T = meta["block_size"]
    start = [t[:, :5].cuda() for t in idx]
    n_new = T + 3 - 5
    a = m.generate(start, max_new_tokens=n_new, modality_to_generate=2, use_cache=True, temperature=0)
    b = m.generate(start, max_new_tokens=n_new, modality_to_generate=2, use_cache=False, temperature=0)
    old = m.generate(start, max_new_tokens=n_new, modality_to_generate=2, use_cache=True,
                     sample_fn=lambda probs: probs.argmax(dim=-1, keepdim=True))
    for i in range(cfg.M):
        assert tuple(a[i].shape) == (start[0].shape[0], T + 3)
        assert torch.equal(a[i], b[i]), i
        assert torch.equal(a[i], old[i]), i


def test_generate_device_shapes_padding_and_unequal_prompts(small, peaked):
    """What test_generate_appends_crops_and_aligns expects of the default path: output shapes, untouched prompts, the
    other modalities padded with their last token; prompts of unequal lengths give what the default path gives."""
    meta, cfg, sd, idx, m = small
    T = meta["block_size"]
    start = [t[:, :10].cuda() for t in idx]
    n_new = T + 8 - 10
    out, lps = m.generate(start, max_new_tokens=n_new, modality_to_generate=1, temperature=1.0, seed=4,
                          return_logprobs=True)
    B = start[0].shape[0]
    for i, o in enumerate(out):
        assert tuple(o.shape) == (B, T + 8) and o.dtype == start[i].dtype, i
        assert torch.equal(o[:, :10], start[i]), i
    gen = out[1][:, 10:]
    assert int(gen.min()) >= 0 and int(gen.max()) < meta["V"][1]
    for i in (0, 2, 3):
        assert torch.equal(out[i][:, 10:], start[i][:, -1:].expand(B, n_new)), i
    assert bool(torch.isfinite(lps).all()) and bool((lps <= 0).all())
    assert tuple(m.generate(start, max_new_tokens=0, temperature=1.0, seed=4)[0].shape) == (B, 10)
    # unequal prompt lengths (all at least block_size, which is what the default path accepts): greedy on the
    # peaked model, against the default path with an argmax sample_fn
    meta, cfg, idx, mp = peaked
    rep = [torch.cat((t, t), dim=1) for t in idx]  # [B, 2 T]
    ragged = [rep[0][:, :T + 5].cuda(), rep[1][:, :T + 2].cuda(), rep[2][:, :T].cuda(), rep[3][:, :T + 9].cuda()]
    new = mp.generate(ragged, max_new_tokens=4, modality_to_generate=1, temperature=0)
    old = mp.generate(ragged, max_new_tokens=4, modality_to_generate=1,
                      sample_fn=lambda probs: probs.argmax(dim=-1, keepdim=True))
    for i in range(cfg.M):
        assert tuple(new[i].shape) == tuple(old[i].shape), i
        assert torch.equal(new[i], old[i]), i


def test_generate_device_path_leaves_torch_generators_alone(small):
    meta, cfg, sd, idx, m = small
    start = [t[:, :6].cuda() for t in idx]
    torch.manual_seed(123)
    cpu0, gpu0 = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    m.generate(start, max_new_tokens=5, modality_to_generate=0, temperature=0.9, top_p=0.8, seed=7)
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), cpu0)
    assert torch.equal(torch.cuda.get_rng_state(), gpu0)
    # seed=None: from the device generator, repeatable under torch.manual_seed, never the CPU generator
    torch.manual_seed(123)
    a = m.generate(start, max_new_tokens=5, modality_to_generate=0, temperature=0.9)
    assert torch.equal(torch.get_rng_state(), cpu0)
    torch.manual_seed(123)
    b = m.generate(start, max_new_tokens=5, modality_to_generate=0, temperature=0.9)
    assert torch.equal(a[0], b[0])


def test_generate_rejects_sample_fn_with_device_keywords(small):
    meta, cfg, sd, idx, m = small
    start = [t[:, :6].cuda() for t in idx]
    fn = lambda probs: probs.argmax(dim=-1, keepdim=True)  # noqa: E731
    for kw in (dict(temperature=1.0), dict(top_k=3), dict(top_p=0.9), dict(seed=1), dict(return_logprobs=True),
               dict(logits_hook=lambda n, lg: None)):
        with pytest.raises(ValueError):
            m.generate(start, max_new_tokens=2, sample_fn=fn, **kw)
    with pytest.raises(ValueError):
        m.generate(start, max_new_tokens=2, temperature=-1.0)
    # the default path is the one that ran before: the CPU generator untouched, the device generator consumed
    torch.manual_seed(5)
    gpu0 = torch.cuda.get_rng_state().clone()
    out = m.generate(start, max_new_tokens=2)
    assert tuple(out[0].shape) == (start[0].shape[0], 8)
    assert not torch.equal(torch.cuda.get_rng_state(), gpu0)
