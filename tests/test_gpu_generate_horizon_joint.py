"""generate(..., horizon={"baskets": ..., "pairs": ...}) on the f_small fixture (d64, L2, T32, V = [57, 13, 24, 5]) with
modalities 1, 2 and 3 generated, all three with values (1 a value series, 2 and 3 percent series), and where evidence is
asked for modality 0 given (its head peaked, as tests/test_gpu_generate_evidence.py does, so the weights differ).

The two keys must leave the run alone: sequences, log-probabilities, `ev` and the per-modality horizon outputs
bit-identical to the same call without them. `joint` must equal, bit for bit, the public mmt_sample.horizon_joint on the
returned sequences and log_weights, and agree with tests/horizon_joint_ref.py under its bounds. Once each on the plain
device path, the fan-out engine, the rolling engine, tiled prompts, evidence="weights" and evidence="resample"."""
import numpy as np
import pytest
import torch

import horizon_joint_ref as J
import mmt_sample as MS
from golden_io import model_fixture
from test_gpu_generate_device import build

pytestmark = pytest.mark.gpu

SEED = 0x101A7
GEN = [1, 2, 3]
PCT = {1: False, 2: True, 3: True}
BARS = {1: [1.0, -1.0], 3: [0.5]}
QUANT = [0.1, 0.5, 0.9]
BASKETS = [{"weights": {1: 1.0, 3: -0.5}, "barriers": [1.0, -1.0]},  # modality 2 not named: coefficient 0
           {"weights": {2: 2.0}, "barriers": [0.5]},
           {"weights": {1: 0.25, 2: 0.25, 3: 0.5}}]


@pytest.fixture(scope="module")
def model():
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    sd = dict(sd)
    sd["post_block.soft_score_layers.0.2.weight"] = sd["post_block.soft_score_layers.0.2.weight"] * 60.0
    m = build(meta, sd)
    m.eval()
    vals = {1: np.linspace(-1.0, 5.0, meta["V"][1]), 2: np.linspace(-3.0, 3.0, meta["V"][2]),
            3: np.array([-2.0, -0.5, 0.0, 0.0, 1.0])}
    return meta, idx, m, vals


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_tree(a, b, where=""):
    """Nested dicts / lists of tensors hold the same bits."""
    if isinstance(a, dict):
        assert sorted(a, key=str) == sorted(b, key=str), where
        for k in a:
            same_tree(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for n, (x, y) in enumerate(zip(a, b)):
            same_tree(x, y, f"{where}/{n}")
    elif isinstance(a, torch.Tensor):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b)), where
    else:
        assert a == b, where


CASES = {"plain": dict(S=None, n0=8, N=12, kw={}),
         "fanout": dict(S=16, n0=8, N=12, kw={}),
         "rolling": dict(S=8, n0=28, N=8, kw=dict(rolling=True)),
         "tiled": dict(S=4, n0=8, N=6, kw=dict(use_cache=False)),
         "weights": dict(S=16, n0=8, N=12, kw=dict(evidence="weights")),
         "resample": dict(S=16, n0=8, N=12, kw=dict(evidence="resample", resample_every=3, ess_threshold=2.0))}


@pytest.mark.parametrize("name", list(CASES))
def test_joint_leaves_the_run_alone_equals_the_public_entry_and_follows_the_rule(model, name):
    meta, idx, m, vals = model
    B, (S, n0, N, extra) = 3, [CASES[name][k] for k in ("S", "n0", "N", "kw")]
    start = [t[:B, :n0].cuda() for t in idx]
    kw = dict(max_new_tokens=N, modality_to_generate=GEN, temperature={1: 0.9}, top_k={3: 3}, seed=SEED,
              return_logprobs=True, num_samples=S, **extra)
    if "evidence" in extra:
        g = torch.Generator().manual_seed(7)
        kw["given"] = {0: torch.randint(0, meta["V"][0], (B, N), generator=g)}
    hz0 = {"values": vals, "is_percent": PCT, "barriers": BARS, "quantiles": QUANT}
    out = m.generate(start, horizon=dict(hz0, baskets=BASKETS, pairs="all"), **kw)  # the present tree refuses the keys
    base = m.generate(start, horizon=hz0, **kw)
    torch.cuda.synchronize()
    if S is not None:
        assert m.last_generate_path == (name if name in ("rolling", "tiled") else "fanout")
    assert len(out) == len(base)
    joint = out[-1]["joint"]
    assert "joint" not in base[-1] and sorted(base[-1]) == GEN
    same_tree(list(out[:-1]), list(base[:-1]), name)
    same_tree({i: out[-1][i] for i in GEN}, base[-1], name + "/hz")

    seqs = out[0]
    logw = out[2]["log_weights"] if "evidence" in extra else None
    Sp = S or 1
    assert joint["modalities"] == GEN and sorted(joint["pairs"]) == [(1, 2), (1, 3), (2, 3)] and len(joint["baskets"]) == 3
    coefs = [[b["weights"].get(i, 0.0) for i in GEN] for b in BASKETS]
    pub = MS.horizon_joint([seqs[i][:, n0:] for i in GEN], samples=Sp, values=[vals[i] for i in GEN],
                           is_percent=[PCT[i] for i in GEN], origin=[seqs[i][:, n0 - 1] for i in GEN], logw=logw,
                           quantiles=QUANT, baskets=[{"weights": c, "barriers": b.get("barriers")}
                                                     for c, b in zip(coefs, BASKETS)], pairs="all")
    same_tree(joint["baskets"], pub["baskets"], name + "/baskets")
    same_tree({(GEN.index(i), GEN.index(k)): v for (i, k), v in joint["pairs"].items()}, pub["pairs"], name + "/pairs")
    same_tree([joint["ess"], joint["live"]], [pub["ess"], pub["live"]], name + "/ess")
    for b, d in zip(BASKETS, joint["baskets"]):
        assert d["hit"].shape == (B, N, len(b.get("barriers", []))) and d["tail_means"].shape == (B, N, 3)
        assert d["stats"].shape == (B, N, 9) and d["quantile_rows"].dtype == torch.int32

    # the rule: one padded number of barriers per call, as generate passes them
    nb = max(len(b.get("barriers", [])) for b in BASKETS)
    bars = [list(b.get("barriers", [])) + [1.0] * (nb - len(b.get("barriers", []))) for b in BASKETS]
    pairs = [(0, 1), (0, 2), (1, 2)]
    problems = [dict(tok=seqs[i][:, n0:].cpu().numpy(), values=vals[i], pct=PCT[i],
                     origin=seqs[i][:, n0 - 1].cpu().numpy()) for i in GEN]
    a = None if logw is None else logw.cpu().numpy()
    refs = J.reference(problems, Sp, coefs, bars, pairs, a, QUANT)
    full = MS.horizon_joint([seqs[i][:, n0:] for i in GEN], samples=Sp, values=[vals[i] for i in GEN],
                            is_percent=[PCT[i] for i in GEN], origin=[seqs[i][:, n0 - 1] for i in GEN], logw=logw,
                            quantiles=QUANT, baskets=[{"weights": c, "barriers": u} for c, u in zip(coefs, bars)],
                            pairs=pairs)
    worst, amb = 0.0, [0, 0, 0]
    for p in range(B):
        got = {"ess": float(full["ess"][p]), "live": int(full["live"][p]),
               "bstats": [d["stats"][p].cpu().numpy() for d in full["baskets"]],
               "bqval": [d["quantile_values"][p].cpu().numpy() for d in full["baskets"]],
               "bqrow": [d["quantile_rows"][p].cpu().numpy() for d in full["baskets"]],
               "btail": [d["tail_means"][p].cpu().numpy() for d in full["baskets"]],
               "bhit": [d["hit"][p].cpu().numpy() for d in full["baskets"]],
               "pstats": [torch.cat([full["pairs"][pq][k][p].reshape(N, -1) for k in (
                   "cov", "corr", "var_p", "var_q", "sign_table", "step_table")], dim=-1).cpu().numpy() for pq in pairs]}
        n_amb, w = J.check(got, refs[p], a is not None, f"{name} prompt {p}")
        worst, amb = max(worst, w), [x + y for x, y in zip(amb, n_amb)]
    if a is not None:
        assert all(n <= J.cap(B * N * 3) for n in amb)
    # the padded call's columns are the cut call's
    for d, e, b in zip(full["baskets"], joint["baskets"], BASKETS):
        same_tree(d["hit"][..., :len(b.get("barriers", []))], e["hit"])
        same_tree(d["stats"], e["stats"])
    if name == "resample":
        assert out[2]["resampled"].any(), "no prompt was resampled"
    print(f"generate horizon joint {name}: max error / bound {worst:.3f}, ambiguous {amb}")


def test_joint_refusals_and_pairs_only(model):
    meta, idx, m, vals = model
    start = [t[:2, :8].cuda() for t in idx]
    ok = {"values": {1: vals[1], 3: vals[3]}, "is_percent": {3: True}}
    for bad in ({"baskets": [{"weights": {2: 1.0}}]},            # modality 2 has no values here
                {"baskets": [{"weights": {1: 0.0}}]}, {"baskets": [{"weights": {1: float("nan")}}]},
                {"pairs": [(1, 1)]}, {"pairs": [(1, 0)]}, {"pairs": "some"}, {"baskets": [], "pairs": []}):
        with pytest.raises(ValueError):
            m.generate(start, max_new_tokens=2, modality_to_generate=GEN, seed=1, horizon=dict(ok, **bad))
    seqs, hz = m.generate(start, max_new_tokens=3, modality_to_generate=GEN, seed=1, horizon=dict(ok, pairs=[(3, 1)]))
    j = hz["joint"]
    assert sorted(hz, key=str) == [1, 3, "joint"] and j["baskets"] == [] and list(j["pairs"]) == [(3, 1)]
    # one path per prompt: every variance is 0, so corr is NaN and each table holds one cell of mass 1
    d = j["pairs"][(3, 1)]
    assert bool(torch.isnan(d["corr"]).all()) and bool((d["cov"] == 0).all()) and bool((j["live"] == 1).all())
    assert bool((d["sign_table"].sum(dim=(2, 3)) == 1).all()) and bool((d["sign_table"].amax(dim=(2, 3)) == 1).all())
