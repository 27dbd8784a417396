"""Engine-level checks of in-place gradient accumulation (MultimodalTransformer.set_grad_accumulation,
mmt_set_grad_accumulate) and of the guarded optimizer step on the model: accumulation against the sum of
the classic path's gradients, bit-reproducibility in deterministic mode, clipping against
torch.nn.utils.clip_grad_norm_ + the plain step, the non-finite skip, main.run with the three config keys,
and data-parallel accumulation under no_sync.

Fixtures are the committed small ones: f_small (d64, T32, B4, cross-attention), f_hs32 (the one-pass hs-32
backward, B2, T64) and f_tiny_v (vocabularies 2 / 1 / 7). Models are built as tests/test_gpu_deterministic_mode.py
builds them, the dropout mask seed pinned.
"""
import functools
import os
import re
import socket
import subprocess
import sys

import pytest
import torch

import config_utils
import mmt_optim
from golden_io import model_fixture

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# the project's bound for "the same sums in another order" (tests/test_gpu_determinism.py)
GRAD_BOUND = 1e-6
PINNED_SEED = 0x5EED1234


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """meta, parameters, micro-batch A (the fixture's batch) and B (its batch rows permuted, every token
    shifted by one inside its vocabulary); made once, never modified."""
    z, meta, cfg, sd, idx, tgt = model_fixture(name)
    B = meta["B"]
    perm = torch.arange(B - 1, -1, -1)
    idx_b = [(t[perm] + 1) % v for t, v in zip(idx, meta["V"])]
    tgt_b = [(t[perm] + 1) % v for t, v in zip(tgt, meta["V"])]
    return meta, sd, (idx, tgt), (idx_b, tgt_b)


def _build(name, det, dropout=0.0):
    meta, sd, _, _ = _fixture(name)
    config_utils._config_cache = {"n_embd": meta["n_embd"], "n_head": meta["n_head"], "n_layer": meta["n_layer"],
                                  "block_size": meta["block_size"], "dropout": dropout, "device": "cuda",
                                  "batch_size": meta["B"], "eval_iters": 1}
    import model as mmt_model
    m = mmt_model.MultimodalTransformer(len(meta["V"]), meta["V"],
                                        [[None] * 8 + [c] + [None] * 3 for c in meta["cross"]]).to("cuda")
    full = {k: t for k, t in m.state_dict().items() if k.endswith("tril")}
    full.update(sd)
    m.load_state_dict(full, strict=True)
    m._next_dropout_seed = lambda dev: PINNED_SEED  # the same masks on every forward
    m.train()
    m.set_deterministic(det)
    return m


def _cuda(batch):
    return [t.cuda() for t in batch[0]], [t.cuda() for t in batch[1]]


def _classic_grad(m, batch):
    """Today's overwriting path: a fresh gradient handed to autograd."""
    m.set_grad_accumulation(False)
    m.flat_params.grad = None
    _, losses = m(*batch)
    sum(losses).backward()
    return m.flat_params.grad.detach().clone()


def _accumulated_grad(m, batches, scale):
    m.set_grad_accumulation(True)
    m.zero_grad(set_to_none=True)
    for b in batches:
        _, losses = m(*b)
        (sum(losses) * scale).backward()
    return m.flat_params.grad.detach().clone()


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------------------------------------ accumulation
@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("name,dropout", [("f_small", 0.0), ("f_small", 0.1), ("f_hs32", 0.0), ("f_tiny_v", 0.0)])
def test_accumulated_gradient_is_the_mean_of_the_micro_batch_gradients(name, dropout, det):
    _, _, A, B = _fixture(name)
    A, B = _cuda(A), _cuda(B)
    m = _build(name, det, dropout)
    gA, gB = _classic_grad(m, A), _classic_grad(m, B)
    assert torch.isfinite(gA).all() and gA.abs().max() > 0 and _rel(gA, gB) > 1e-2  # two different micro-batches
    g_acc = _accumulated_grad(m, [A, B], 0.5)
    want = (gA + gB) / 2
    err = _rel(g_acc, want)
    print(f"{name} dropout {dropout} det {det}: accumulated vs mean of classic gradients rel-L2 {err:.3e}")
    assert err <= GRAD_BOUND, err
    assert m.flat_params.grad.data_ptr() == m._grad_buf.data_ptr()  # in place: the model's own buffer
    # reference_grad_views() keeps working on the accumulated gradient
    views = {k: g for k, g in m.reference_grad_views() if g is not None}
    assert len(views) == sum(1 for t in m._tensors if t[1] < m._n_active)
    for k0, off0, shp0, _ in (m._tensors[0], m._tensors[-1]):
        if k0 in views:
            assert torch.equal(views[k0], g_acc[off0:off0 + views[k0].numel()].view(shp0))
    if det:
        again = _accumulated_grad(m, [A, B], 0.5)  # .grad from None: the buffer is overwritten, then added to
        assert torch.equal(again, g_acc), f"{int((again != g_acc).sum())} entries differ between two accumulated runs"


@pytest.mark.parametrize("name", ["f_small", "f_hs32", "f_tiny_v"])
def test_first_in_place_backward_equals_the_classic_gradient(name):
    """Accumulation on and .grad None: the engine overwrites the model's buffer, whatever it held."""
    _, _, A, B = _fixture(name)
    A, B = _cuda(A), _cuda(B)
    m = _build(name, True, 0.1)
    gA = _classic_grad(m, A)
    _accumulated_grad(m, [B, B], 1.0)  # leaves another gradient in the model's buffer
    m.zero_grad(set_to_none=True)
    assert m.flat_params.grad is None
    got = _accumulated_grad(m, [A], 1.0)
    assert torch.equal(got, gA), f"{int((got != gA).sum())} of {gA.numel()} entries differ"


def test_in_place_mode_returns_no_gradient_to_autograd():
    _, _, A, _ = _fixture("f_small")
    A = _cuda(A)
    m = _build("f_small", True)
    seen = []
    m.flat_params.register_hook(lambda g: seen.append(g))
    gA = _classic_grad(m, A)
    assert len(seen) == 1 and torch.equal(seen[0], gA)
    got = _accumulated_grad(m, [A], 1.0)
    # documented: autograd has no gradient for flat_params in this mode, so a tensor hook on it gets none
    # (torch does not call it, or calls it with None, depending on the version); AccumulateGrad adds nothing
    assert all(g is None for g in seen[1:])
    assert torch.equal(got, gA) and m.flat_params.grad.data_ptr() == m._grad_buf.data_ptr()


# ------------------------------------------------------------------------------------------------ clipping
def test_clipping_matches_clip_grad_norm_and_the_plain_step():
    """Two copies in deterministic mode on identical data (identical gradients): torch's clip_grad_norm_ +
    the plain AdamW against AdamW(max_grad_norm=c). One step: norms to 1e-6, updates to rel-L2 1e-6 (a
    relative perturbation of a few ulps on g). Six steps: losses to 1e-5 relative.
    Measured on MI355X: norms 1.0e-7 apart, first update 2.1e-7, losses at most 3.1e-6 apart over the six steps."""
    _, _, A, _ = _fixture("f_small")
    A = _cuda(A)
    m1, m2 = _build("f_small", True, 0.1), _build("f_small", True, 0.1)
    norm0 = _classic_grad(m1, A).norm().item()
    c = 0.5 * norm0
    m1.flat_params.grad = None
    p0 = m1.flat_params.detach().clone()
    o1 = mmt_optim.AdamW(m1.parameters(), lr=1e-3)
    o2 = mmt_optim.AdamW(m2.parameters(), lr=1e-3, max_grad_norm=c)
    hist = []
    for step in range(6):
        _, l1 = m1(*A)
        o1.zero_grad(set_to_none=True)
        sum(l1).backward()
        tn = torch.nn.utils.clip_grad_norm_(m1.parameters(), c)
        o1.step()
        _, l2 = m2(*A)
        o2.zero_grad(set_to_none=True)
        sum(l2).backward()
        o2.step()
        l1, l2 = torch.stack([x.detach() for x in l1]), torch.stack([x.detach() for x in l2])
        hist.append(((l1 - l2).abs() / l1.abs()).max().item())
        if step == 0:
            assert torch.equal(l1, l2)
            got = float(o2.last_grad_norm)
            assert got > c  # the step was clipped
            assert abs(got - float(tn)) <= 1e-6 * float(tn), (got, float(tn))
            u1, u2 = m1.flat_params.detach() - p0, m2.flat_params.detach() - p0
            err = _rel(u2, u1)
            print(f"step 1: norm {got!r} vs torch {float(tn)!r}, update rel-L2 {err:.3e}")
            assert err <= 1e-6, err
    print("loss rel differences per step:", " ".join(f"{h:.2e}" for h in hist))
    assert hist[-1] <= 1e-5, hist
    assert o2.counters()[0] == 6 and o2.counters()[1] == 0 and o2.counters()[2] >= 1


# ------------------------------------------------------------------------------------------------ skip
def test_nonfinite_gradient_skips_the_model_step():
    _, _, A, _ = _fixture("f_small")
    A = _cuda(A)
    m = _build("f_small", True)
    opt = mmt_optim.AdamW(m.parameters(), lr=1e-3, skip_nonfinite=True)
    # one clean step first, so the moments are not zero
    _, losses = m(*A)
    sum(losses).backward()
    opt.step()
    st = opt.state[m.flat_params]
    before = [m.flat_params.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    mask0 = int(m.nonfinite_loss_mask().item())
    opt.zero_grad(set_to_none=True)
    _, losses = m(*A)
    sum(losses).backward()
    m.flat_params.grad[12345 % m.flat_params.numel()] = float("nan")
    opt.step()
    after = [m.flat_params.detach(), st["exp_avg"], st["exp_avg_sq"]]
    for a, b in zip(after, before):
        assert torch.equal(a, b)
    assert int(m.nonfinite_loss_mask().item()) == mask0 == 0  # the loss flag is another matter: the losses were finite
    assert opt.counters() == (1, 1, 0)
    # and as the very first step
    m2 = _build("f_small", True)
    opt2 = mmt_optim.AdamW(m2.parameters(), lr=1e-3, skip_nonfinite=True, max_grad_norm=1.0)
    p0 = m2.flat_params.detach().clone()
    _, losses = m2(*A)
    sum(losses).backward()
    m2.flat_params.grad[0] = float("nan")
    opt2.step()
    st2 = opt2.state[m2.flat_params]
    assert torch.equal(m2.flat_params.detach(), p0)
    assert not st2["exp_avg"].any() and not st2["exp_avg_sq"].any()
    assert opt2.counters() == (0, 1, 0)


# ------------------------------------------------------------------------------------------------ main.run
def test_main_run_with_clip_accumulation_and_skip(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.dirname(HERE))
    import main
    import mmt_data
    cfg = config_utils.load_system_config("/nonexistent.yaml")
    cfg.update({"device": "cuda", "batch_size": 4, "block_size": 32, "max_iters": 5, "eval_interval": 2,
                "eval_iters": 1, "learning_rate": 3e-3, "n_embd": 64, "n_head": 2, "n_layer": 1, "dropout": 0.0,
                "project_file_path": str(tmp_path) + "/", "output_file_name": "", "model_file_name": "m.pth",
                "save_model": 0, "create_new_model": 1,
                "grad_clip": 0.5, "grad_accum_steps": 2, "skip_nonfinite_steps": True})
    calls = []
    real = main.get_batch
    monkeypatch.setattr(main, "get_batch", lambda *a, **k: (calls.append(a), real(*a, **k))[1])
    data = mmt_data.make_synthetic(n_rows=20_000, n_files=5)
    lines = []
    m, hist = main.run(dict(cfg), data, log=lines.append)
    text = "\n".join(lines)
    assert "TRAINING COMPLETED SUCCESSFULLY" in text
    assert [h[0] for h in hist] == [0, 2, 4]
    assert all(torch.isfinite(torch.tensor([h[1], h[2]])).all() for h in hist)
    assert len(calls) == 2 * cfg["max_iters"]  # two micro-batches per iteration
    assert m.grad_accumulation is True
    evals = re.findall(r"LOSS METRICS: Step (\d+)/5 .*\| GradNorm: (n/a|[0-9.]+) \| Clipped: (\d+) \| Skipped: (\d+) \| Time:",
                       text)
    assert [e[0] for e in evals] == ["0", "2", "4"], text
    assert evals[0][1:] == ("n/a", "0", "0")  # nothing stepped yet
    assert float(evals[1][1]) > 0 and float(evals[2][1]) > 0
    assert sum(int(e[2]) for e in evals) <= 4 and all(e[3] == "0" for e in evals)


def test_main_run_reports_the_counts_when_an_evaluation_is_nan(tmp_path, monkeypatch):
    """An evaluation with NaN losses prints no LOSS METRICS line: its warning line carries the norm and
    the counts of that interval instead, so they are never dropped."""
    sys.path.insert(0, os.path.dirname(HERE))
    import main
    import mmt_data
    cfg = config_utils.load_system_config("/nonexistent.yaml")
    cfg.update({"device": "cuda", "batch_size": 4, "block_size": 32, "max_iters": 5, "eval_interval": 2,
                "eval_iters": 1, "learning_rate": 3e-3, "n_embd": 64, "n_head": 2, "n_layer": 1, "dropout": 0.0,
                "project_file_path": str(tmp_path) + "/", "output_file_name": "", "model_file_name": "m.pth",
                "save_model": 0, "create_new_model": 1, "grad_clip": 1e-3})
    real = main.estimate_loss
    nan = float("nan")
    monkeypatch.setattr(main, "estimate_loss",
                        lambda it, n: {"train": nan, "val": nan} if it == 2 else real(it, n))
    lines = []
    main.run(dict(cfg), mmt_data.make_synthetic(n_rows=20_000, n_files=5), log=lines.append)
    text = "\n".join(lines)
    note = r"\| GradNorm: ([0-9.]+) \| Clipped: (\d+) \| Skipped: (\d+) \| "
    warn = re.search(r"Warning: Step 2 losses are NaN, skipping save " + note, text)
    assert warn and warn.group(2) == "2" and warn.group(3) == "0", text  # steps 0 and 1, both clipped at 1e-3
    last = re.search(r"LOSS METRICS: Step 4/5 .*" + note + "Time:", text)
    assert last and last.group(2) == "2", text  # steps 2 and 3 only


def test_main_run_default_log_lines_are_unchanged(tmp_path):
    sys.path.insert(0, os.path.dirname(HERE))
    import main
    import mmt_data
    cfg = config_utils.load_system_config("/nonexistent.yaml")
    cfg.update({"device": "cuda", "batch_size": 4, "block_size": 32, "max_iters": 3, "eval_interval": 2,
                "eval_iters": 1, "learning_rate": 3e-3, "n_embd": 64, "n_head": 2, "n_layer": 1, "dropout": 0.0,
                "project_file_path": str(tmp_path) + "/", "output_file_name": "", "model_file_name": "m.pth",
                "save_model": 0, "create_new_model": 1})
    lines = []
    m, _ = main.run(dict(cfg), mmt_data.make_synthetic(n_rows=20_000, n_files=5), log=lines.append)
    text = "\n".join(lines)
    assert "GradNorm" not in text and re.search(r"LOSS METRICS: Step 2/3 \| Train: [0-9.]+ \| Val: [0-9.]+ \| Time:", text)
    assert m.grad_accumulation is False


# ------------------------------------------------------------------------------------------------ data parallel
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_dp_accumulation_under_no_sync_matches_single_process():
    """tests/workers/dp_accumulation.py: 2 gloo ranks on one GPU, two micro-batches each (the first under
    no_sync), against one process accumulating the same four micro-batches at loss scale 1/4."""
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "2"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(HERE, "workers", "dp_accumulation.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=100)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0
    assert "rank 0 ok" in r.stdout and "rank 1 ok" in r.stdout
