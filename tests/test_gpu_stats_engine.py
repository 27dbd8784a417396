"""Engine-level checks of the per-tensor statistics on the f_small model (d64, T32, B4, cross-attention; built
as tests/test_gpu_guard_engine.py builds it): model.tensor_stats against the reference tensor views, the
first-skipped-step record through mmt_optim.AdamW(stats=...), mode "every", and main.run's GRAD STATS line.

Bounds: absmax, the counts and first_bad are exact; sqsum of a tensor of k elements is within k * 2^-53 relative
of math.fsum over the fp64 squares (tests/test_gpu_stats_kernels.py derives it); the report's global norm agrees
with the guard's to NORM_BOUND, the project's 2 fp32 ulps (tests/test_gpu_guard_kernels.py).
"""
import functools
import math
import os
import re
import sys

import pytest
import torch

import config_utils
import mmt_optim
import mmt_stats
from golden_io import model_fixture

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
NORM_BOUND = 2.4e-7
PINNED_SEED = 0x5EED1234


@functools.lru_cache(maxsize=None)
def _fixture():
    """meta, parameters, micro-batch A (the fixture's) and B (rows permuted, tokens shifted); never modified."""
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    perm = torch.arange(meta["B"] - 1, -1, -1)
    idx_b = [(t[perm] + 1) % v for t, v in zip(idx, meta["V"])]
    tgt_b = [(t[perm] + 1) % v for t, v in zip(tgt, meta["V"])]
    return meta, sd, (idx, tgt), (idx_b, tgt_b)


def _build():
    meta, sd, _, _ = _fixture()
    config_utils._config_cache = {"n_embd": meta["n_embd"], "n_head": meta["n_head"], "n_layer": meta["n_layer"],
                                  "block_size": meta["block_size"], "dropout": 0.0, "device": "cuda",
                                  "batch_size": meta["B"], "eval_iters": 1}
    import model as mmt_model
    m = mmt_model.MultimodalTransformer(len(meta["V"]), meta["V"],
                                        [[None] * 8 + [c] + [None] * 3 for c in meta["cross"]]).to("cuda")
    full = {k: t for k, t in m.state_dict().items() if k.endswith("tril")}
    full.update(sd)
    m.load_state_dict(full, strict=True)
    m._next_dropout_seed = lambda dev: PINNED_SEED
    m.train()
    m.set_deterministic(True)
    return m


def _batch(which):
    b = _fixture()[2 + which]
    return [t.cuda() for t in b[0]], [t.cuda() for t in b[1]]


def _backward(m, opt, batch):
    opt.zero_grad(set_to_none=True)
    _, losses = m(*batch)
    sum(losses).backward()


def _check_against_views(rep, views):
    """views: {name: tensor} of every named tensor. Returns the worst sqsum error in units of its bound."""
    assert sorted(rep.names) == sorted(views)
    worst = 0.0
    for i, name in enumerate(rep.names):
        v = views[name].detach().double().flatten().cpu()
        ref = math.fsum((v * v).tolist())
        got = float(rep.sqsum[i])
        err = abs(got - ref) / ref if ref > 0 else abs(got)
        worst = max(worst, err / (v.numel() * U))
        assert err <= v.numel() * U, (name, got, ref)
        assert float(rep.absmax[i]) == float(views[name].detach().abs().max()), name
        assert (int(rep.nan_count[i]), int(rep.inf_count[i]), int(rep.first_bad[i])) == (0, 0, -1), name
    return worst


# ------------------------------------------------------------------------------------------------ healthy run
def test_tensor_stats_of_a_healthy_step():
    m = _build()
    opt = mmt_optim.AdamW(m.parameters(), lr=1e-3, max_grad_norm=float("inf"))
    seg = m.tensor_segments()
    assert seg is m.tensor_segments() and seg["device"].is_cuda  # made once
    assert len(seg["names"]) == sum(1 for t in m._tensors if t[1] < m._n_active) > 10
    assert all(e <= b2 for e, b2 in zip(seg["ends"], seg["begins"][1:]))  # disjoint, in offset order
    _backward(m, opt, _batch(0))
    rep = m.tensor_stats("grad")
    views = {k: g for k, g in m.reference_grad_views() if g is not None}
    worst = _check_against_views(rep, views)
    opt.step()
    norm = float(opt.last_grad_norm)
    print(f"grad: {len(rep.names)} tensors, worst sqsum error {worst:.3f} of its bound; global norm "
          f"{rep.global_norm!r} vs guard {norm!r}")
    assert rep.global_norm > 0 and abs(rep.global_norm - norm) <= NORM_BOUND * norm
    stages = rep.by_stage()
    assert len(stages) == len(m.backward_stage_ranges()) and sum(s["tensors"] for s in stages) == len(rep.names)
    assert all(s["nonfinite"] == 0 for s in stages) and rep.first_poisoned_stage is None
    assert abs(math.sqrt(sum(s["norm"] ** 2 for s in stages)) - rep.global_norm) <= 1e-12 * rep.global_norm
    # the parameters, after the step
    repp = m.tensor_stats("param")
    active = set(seg["names"])
    _check_against_views(repp, {k: v for k, v in m.named_reference_tensors() if k in active})
    with pytest.raises(ValueError):
        m.tensor_stats("moments")


# ------------------------------------------------------------------------------------------------ mode "skipped"
def _poison(m, name, k):
    view = dict(m.reference_grad_views())[name]
    view.view(-1)[k] = float("nan")


def test_skipped_mode_names_the_poisoned_tensor_and_keeps_the_first_record():
    m = _build()
    stats = mmt_stats.TensorStats(m, "skipped")
    opt = mmt_optim.AdamW(m.parameters(), lr=1e-3, skip_nonfinite=True, stats=stats)
    seg = m.tensor_segments()
    layer0 = [n for n, b, e in zip(seg["names"], seg["begins"], seg["ends"]) if n.startswith("blocks.0.") and e - b > 40]
    first, second = layer0[0], layer0[-1]
    assert first != second
    A, B = _batch(0), _batch(1)
    _backward(m, opt, A)
    opt.step()  # one clean step first, so the moments are not zero
    assert stats.read() is None
    st = opt.state[m.flat_params]
    before = [m.flat_params.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    _backward(m, opt, A)
    _poison(m, first, 37)
    opt.step()
    for a, b in zip([m.flat_params.detach(), st["exp_avg"], st["exp_avg_sq"]], before):
        assert torch.equal(a, b)  # skipped: nothing moved
    snapshot = stats._rec.clone()
    # further clean steps and a second, different faulty step leave the record alone
    for batch in (B, A):
        _backward(m, opt, batch)
        opt.step()
    _backward(m, opt, B)
    _poison(m, second, 5)
    opt.step()
    assert opt.counters()[:2] == (3, 2)
    assert torch.equal(stats._rec, snapshot)
    rep = stats.read(rearm=True)
    assert rep.nonfinite() == [(first, 1, 0, 37)]
    assert (rep.applied_steps, rep.skipped_steps) == (1, 1)
    begin = seg["begins"][seg["names"].index(first)]
    want_stage = next(s for s, (lo, hi) in enumerate(m.backward_stage_ranges()) if lo <= begin < hi)
    assert rep.first_poisoned_stage == want_stage
    line = rep.format()
    assert f"non-finite tensors: 1/{len(rep.names)}" in line and first in line and "applied 1 skipped 1" in line
    # the finite statistics of that step are there too: every other tensor's absmax is a real gradient's
    assert (rep.absmax > 0).sum() >= len(rep.names) // 2
    # re-armed: the next faulty step is recorded
    assert stats.read() is None
    _backward(m, opt, A)
    _poison(m, second, 5)
    opt.step()
    rep2 = stats.read()
    assert rep2.nonfinite() == [(second, 1, 0, 5)]
    assert (rep2.applied_steps, rep2.skipped_steps) == (3, 3)


# ------------------------------------------------------------------------------------------------ mode "every"
def test_every_mode_follows_the_latest_step():
    m = _build()
    stats = mmt_stats.TensorStats(m, "every")
    opt = mmt_optim.AdamW(m.parameters(), lr=1e-3, max_grad_norm=1.0, stats=stats)
    _backward(m, opt, _batch(0))
    opt.step()
    r1 = stats.read(rearm=False)
    assert (r1.applied_steps, r1.skipped_steps) == (1, 0)
    assert abs(r1.global_norm - float(opt.last_grad_norm)) <= NORM_BOUND * r1.global_norm
    _backward(m, opt, _batch(1))
    opt.step()
    r2 = stats.read(rearm=False)
    assert (r2.applied_steps, r2.skipped_steps) == (2, 0)
    assert abs(r2.global_norm - float(opt.last_grad_norm)) <= NORM_BOUND * r2.global_norm
    assert (r1.sqsum != r2.sqsum).sum() > len(r1.names) // 2  # another batch: another gradient
    _check_against_views(r2, {k: g for k, g in m.reference_grad_views() if g is not None})
    # the plain optimizer takes mode "every" too, and refuses mode "skipped"
    plain = mmt_optim.AdamW(m.parameters(), lr=1e-3, stats=mmt_stats.TensorStats(m, "every"))
    plain.step()
    r3 = plain.stats.read()
    assert torch.equal(torch.from_numpy(r3.sqsum), torch.from_numpy(r2.sqsum)) and r3.applied_steps == 0
    with pytest.raises(ValueError):
        mmt_optim.AdamW(m.parameters(), lr=1e-3, stats=mmt_stats.TensorStats(m, "skipped"))


# ------------------------------------------------------------------------------------------------ main.run
def _tiny_cfg(tmp_path, **extra):
    cfg = config_utils.load_system_config("/nonexistent.yaml")
    cfg.update({"device": "cuda", "batch_size": 4, "block_size": 32, "max_iters": 5, "eval_interval": 2,
                "eval_iters": 1, "learning_rate": 3e-3, "n_embd": 64, "n_head": 2, "n_layer": 1, "dropout": 0.0,
                "project_file_path": str(tmp_path) + "/", "output_file_name": "", "model_file_name": "m.pth",
                "save_model": 0, "create_new_model": 1})
    cfg.update(extra)
    return cfg


def test_main_run_logs_grad_stats_only_when_asked(tmp_path):
    sys.path.insert(0, os.path.dirname(HERE))
    import main
    import mmt_data
    data = mmt_data.make_synthetic(n_rows=20_000, n_files=5)
    lines = []
    main.run(dict(_tiny_cfg(tmp_path, grad_stats="every")), data, log=lines.append)
    text = "\n".join(lines)
    assert "TRAINING COMPLETED SUCCESSFULLY" in text
    got = [l for l in lines if "GRAD STATS" in l]
    assert all(l.startswith("GRAD STATS: ") for l in got)
    found = [re.match(r"GRAD STATS: Step (\d+)/5 \| applied (\d+) skipped 0 \| norm: ([0-9.]+) \| tensors: \d+ \| "
                      r"largest: \S+ [0-9.e+-]+, \S+ [0-9.e+-]+, \S+ [0-9.e+-]+$", l) for l in got]
    assert all(found), got
    # evaluations at 0, 2, 4: nothing has stepped at 0; afterwards one line each, of the latest step
    assert [(f.group(1), f.group(2)) for f in found] == [("2", "2"), ("4", "4")], got
    assert all(float(f.group(3)) > 0 for f in found)
    assert len(re.findall(r"LOSS METRICS: Step \d+/5 .*\| GradNorm: ", text)) == 3  # guarded, as accumulation alone is
    lines = []
    cfg = _tiny_cfg(tmp_path, max_iters=3)
    assert "grad_stats" in cfg and cfg.pop("grad_stats") == "off"  # the key absent
    main.run(dict(cfg), data, log=lines.append)
    assert not any("GRAD STATS" in l for l in lines)
    assert not any("GradNorm" in l for l in lines)
