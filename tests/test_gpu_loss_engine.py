"""Engine-level checks of the training objective (MultimodalTransformer.set_loss -> mmt_set_loss) on the f_small
model (d64, T32, B4, cross-attention; built as tests/test_gpu_stats_engine.py builds it, deterministic mode).

Bounds. The losses against tests/loss_ref.py on the engine's OWN fp32 logits: rtol = atol = 1e-5, the loss
kernel's bound (tests/test_gpu_loss_kernel.py). The losses and gradients against the CPU oracle
(oracle/mmt_oracle.py forward on leaf copies of the parameters, the loss_ref objective, autograd): the bf16
tolerances tests/test_gpu_model.py states in its header: losses 5e-3, all gradients together rel-L2 <= 3e-2, every
tensor rel-L2 <= 1e-1 or abs-L2 <= 2e-3 of the whole gradient's norm."""
import ctypes
import functools
import os
import sys

import pytest
import torch

import config_utils
import loss_ref
import mmt_lib as ML
from golden_io import model_fixture

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PINNED_SEED = 0x5EED1234
GRAD_TOL = 3e-2


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _build(name="f_small", train=True):
    z, meta, cfg, sd, idx, tgt = model_fixture(name)
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
    m.train(train)
    m.set_deterministic(True)
    return m, [t.cuda() for t in idx], [t.cuda() for t in tgt]


def _spec(meta):
    """eps = 0.1, class weights in [0.2, 1.2], position weights 0 on the first quarter and a ramp behind it."""
    T = meta["block_size"]
    g = torch.Generator().manual_seed(11)
    cw = {i: torch.rand(v, generator=g) + 0.2 for i, v in enumerate(meta["V"])}
    u = torch.zeros(T)
    u[T // 4:] = torch.linspace(0.5, 1.5, T - T // 4)
    return 0.1, cw, u


def _step(m, idx, tgt):
    m.flat_params.grad = None
    logits, losses = m(idx, tgt)
    sum(losses).backward()
    torch.cuda.synchronize()
    return [l.clone() for l in logits], torch.stack([l.detach() for l in losses]).clone(), m.flat_params.grad.clone()


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _plain_step():
    m, idx, tgt = _build()
    return _step(m, idx, tgt)


@functools.lru_cache(maxsize=None)
def _spec_step():
    m, idx, tgt = _build()
    meta = model_fixture("f_small")[1]
    m.set_loss(*_spec(meta))
    return _step(m, idx, tgt), {k: (None if g is None else g.detach().cpu().clone()) for k, g in m.reference_grad_views()}


@functools.lru_cache(maxsize=None)
def _oracle(with_spec):
    """losses and gradients of the CPU oracle under the loss_ref objective (or the plain mean CE)."""
    import mmt_oracle as O
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    eps, cw, u = _spec(meta)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    logits, _ = O.forward(leaves, cfg, idx)
    T = meta["block_size"]
    losses = []
    for i, lg in enumerate(logits):
        x, t = lg.view(-1, lg.shape[-1]), tgt[i].reshape(-1)
        losses.append(loss_ref.objective(x, t, T, eps, cw[i], u) if with_spec else loss_ref.objective(x, t, T))
    sum(losses).backward()
    return torch.stack([l.detach() for l in losses]), {k: v.grad for k, v in leaves.items()}


# ------------------------------------------------------------------------------------------------ (a), (b), (d)
def test_set_loss_then_plain_is_bit_identical_to_never_having_a_spec():
    logits0, losses0, grad0 = _plain_step()
    m, idx, tgt = _build()
    meta = model_fixture("f_small")[1]
    m.set_loss(*_spec(meta))
    _, losses_s, _ = _step(m, idx, tgt)
    assert not torch.equal(losses_s, losses0)
    m.set_loss()
    assert m.loss_spec is None
    logits1, losses1, grad1 = _step(m, idx, tgt)
    assert torch.equal(_bits(losses1), _bits(losses0))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(logits1, logits0))
    assert torch.equal(_bits(grad1), _bits(grad0))


def test_spec_leaves_the_logits_alone_and_repeats_bit_for_bit():
    logits0, _, _ = _plain_step()
    (logits1, losses1, grad1), _ = _spec_step()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(logits1, logits0))
    m, idx, tgt = _build()
    m.set_loss(*_spec(model_fixture("f_small")[1]))
    _, losses2, grad2 = _step(m, idx, tgt)
    assert torch.equal(_bits(losses2), _bits(losses1))
    assert torch.equal(_bits(grad2), _bits(grad1))
    _, losses3, grad3 = _step(m, idx, tgt)  # ... and on the same model again
    assert torch.equal(_bits(losses3), _bits(losses1)) and torch.equal(_bits(grad3), _bits(grad1))


# ------------------------------------------------------------------------------------------------ (c)
def test_losses_and_gradients_against_the_references():
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    eps, cw, u = _spec(meta)
    T = meta["block_size"]
    o_losses, o_grads = _oracle(True)
    p_losses, p_grads = _oracle(False)
    keys = [k for k in o_grads if o_grads[k] is not None and k not in set(meta["grad_none"])]
    allr = torch.cat([o_grads[k].flatten() for k in keys])
    allp = torch.cat([p_grads[k].flatten() for k in keys])
    moved = rel(allp, allr)
    print(f"reference: the spec moves the gradient by rel-L2 {moved:.3f}; losses {o_losses.tolist()} plain {p_losses.tolist()}")
    assert moved >= 10 * GRAD_TOL  # the plain loss cannot pass below

    (logits, losses, _), grads = _spec_step()
    # the loss kernel on the engine's own logits
    for i, lg in enumerate(logits):
        ref = loss_ref.objective(lg.view(-1, lg.shape[-1]), tgt[i].reshape(-1).cuda(), T, eps, cw[i], u)
        print(f"modality {i}: loss {float(losses[i]):.8f} loss_ref on the engine's logits {float(ref):.8f}")
        torch.testing.assert_close(losses[i].double(), ref, rtol=1e-5, atol=1e-5)
    # the whole step against the oracle
    assert torch.allclose(losses.cpu().double(), o_losses, rtol=5e-3, atol=5e-3), (losses, o_losses)
    allg = torch.cat([grads[k].flatten() for k in keys])
    gnorm = allr.norm().item()
    err = rel(allg, allr)
    print(f"all gradients rel-L2 {err:.4f} (against the plain reference: {rel(allg, allp):.4f})")
    assert err < GRAD_TOL
    for k in keys:
        if grads[k].numel() == 0:
            continue
        e = (grads[k].double() - o_grads[k].double()).norm().item()
        assert e <= 0.1 * o_grads[k].norm().item() or e <= 2e-3 * gnorm, (k, e, gnorm)
    for k in meta["grad_none"]:
        assert grads[k] is None


# ------------------------------------------------------------------------------------------------ (e)
LABELS = ["ce_fwd", "ce_denom"]


def _counts(m, step):
    L = ML.lib()
    L.mmt_probe_set(m._ctx, ",".join(LABELS).encode())
    L.mmt_probe_enable(m._ctx, 1)
    try:
        step()
        torch.cuda.synchronize()
        out = {}
        for i, lab in enumerate(LABELS):
            ms, n, fl, by = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
            ML.check(L.mmt_probe_read_at(m._ctx, i, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by)),
                     m._ctx, "mmt_probe_read_at")
            out[lab] = n.value
        return out
    finally:
        L.mmt_probe_set(m._ctx, None)


def test_launch_counts():
    m, idx, tgt = _build()
    meta = model_fixture("f_small")[1]
    eps, cw, u = _spec(meta)

    def step():
        m.flat_params.grad = None
        _, losses = m(idx, tgt)
        sum(losses).backward()

    assert _counts(m, step) == {"ce_fwd": 1, "ce_denom": 0}
    m.set_loss(eps)
    assert _counts(m, step) == {"ce_fwd": 1, "ce_denom": 0}  # eps alone: D = R, no pre-pass
    m.set_loss(eps, cw, u)
    assert _counts(m, step) == {"ce_fwd": 1, "ce_denom": 1}
    m.set_loss(0.0, {1: cw[1]})
    assert _counts(m, step) == {"ce_fwd": 1, "ce_denom": 1}
    m.set_loss()
    assert _counts(m, step) == {"ce_fwd": 1, "ce_denom": 0}


# ------------------------------------------------------------------------------------------------ (f)
def test_eval_mode_forward_returns_the_same_objective():
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    eps, cw, u = _spec(meta)
    T = meta["block_size"]
    (_, train_losses, _), _ = _spec_step()
    m, idx_d, tgt_d = _build(train=False)
    m.set_loss(eps, cw, u)
    with torch.no_grad():
        logits, losses = m(idx_d, tgt_d)
    torch.cuda.synchronize()
    for i, lg in enumerate(logits):
        ref = loss_ref.objective(lg.view(-1, lg.shape[-1]), tgt_d[i].reshape(-1), T, eps, cw[i], u)
        torch.testing.assert_close(losses[i].double(), ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(torch.stack(list(losses)), train_losses, rtol=5e-3, atol=5e-3)  # dropout 0: one forward


# ------------------------------------------------------------------------------------------------ (g)
def test_tiny_vocabularies():
    z, meta, cfg, sd, idx, tgt = model_fixture("f_tiny_v")
    assert sorted(meta["V"]) == [1, 2, 7]
    m, idx_d, tgt_d = _build("f_tiny_v")
    T = meta["block_size"]
    _, plain, _ = _step(m, idx_d, tgt_d)
    m.set_loss(0.1)
    logits, losses, grad = _step(m, idx_d, tgt_d)
    assert torch.isfinite(losses).all() and torch.isfinite(grad).all()
    for i, lg in enumerate(logits):
        ref = loss_ref.objective(lg.view(-1, lg.shape[-1]), tgt_d[i].reshape(-1), T, 0.1)
        torch.testing.assert_close(losses[i].double(), ref, rtol=1e-5, atol=1e-5)
        if meta["V"][i] == 1:
            assert float(losses[i]) == 0.0  # one class: nothing to smooth
        else:
            assert float(losses[i]) != float(plain[i])
    assert int(m.nonfinite_loss_mask().item()) == 0


# ------------------------------------------------------------------------------------------------ (h)
def _tiny_cfg(tmp_path, **extra):
    cfg = config_utils.load_system_config("/nonexistent.yaml")
    cfg.update({"device": "cuda", "batch_size": 4, "block_size": 32, "max_iters": 3, "eval_interval": 2,
                "eval_iters": 1, "learning_rate": 3e-3, "n_embd": 64, "n_head": 2, "n_layer": 1, "dropout": 0.0,
                "project_file_path": str(tmp_path) + "/", "output_file_name": "", "model_file_name": "m.pth",
                "save_model": 0, "create_new_model": 1, "deterministic": True})
    cfg.update(extra)
    return cfg


def test_main_run_with_the_config_keys(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.dirname(HERE))
    import main
    import mmt_data
    import mmt_loss
    data = mmt_data.make_synthetic(n_rows=20_000, n_files=5)
    V = data["vocab_sizes"]
    by_hand = {i: mmt_loss.balanced_class_weights(data["train"][i], V[i], 1.0) for i in range(len(V))}
    record = []  # (training, parameters, idx, tgt, losses) of every forward with targets

    Plain = main.MultimodalTransformer

    class Recording(Plain):
        def forward(self, idx_list, targets_list=None):
            before = self.flat_params.detach().clone()
            out = super().forward(idx_list, targets_list)
            if targets_list is not None:
                record.append((self.training, before, [t.clone() for t in idx_list], [t.clone() for t in targets_list],
                               torch.stack([l.detach() for l in out[1]]).clone()))
            return out

    monkeypatch.setattr(main, "MultimodalTransformer", Recording)
    lines = []
    cfg = _tiny_cfg(tmp_path, label_smoothing=0.1, loss_class_weights="balanced")
    main.run(dict(cfg), data, log=lines.append)
    got = [l for l in lines if "LOSS OBJECTIVE" in l]
    assert len(got) == 1 and got[0].startswith("LOSS OBJECTIVE: label_smoothing 0.1 | class weights balanced (power 1; "), got
    assert got[0].endswith("positions from 0 of 32")
    assert "TRAINING COMPLETED SUCCESSFULLY" in "\n".join(lines)
    steps = [r for r in record if r[0]]
    assert len(steps) == 3 and len(record) > 3  # three training steps and the evaluations
    assert all(torch.isfinite(r[4]).all() for r in record)
    # the same steps by hand: a model of the same shape, that step's parameters, set_loss with the weights above
    config_utils._config_cache = dict(cfg)
    hand = Plain(len(V), V, data["params"]).to("cuda")
    hand.set_deterministic(True)
    hand.set_loss(0.1, by_hand)
    for training, params, idx, tgt, losses in record:
        with torch.no_grad():
            hand.flat_params.copy_(params)
        hand.train(training)
        with torch.no_grad():
            _, l = hand(idx, tgt)
        assert torch.equal(_bits(torch.stack(list(l))), _bits(losses))
    hand.set_loss()
    with torch.no_grad():
        _, l = hand(record[-1][2], record[-1][3])
    assert not torch.equal(torch.stack(list(l)), record[-1][4])  # ... and the plain loss is another number

    # the keys absent: no line, no import needed, the plain losses
    lines = []
    cfg = _tiny_cfg(tmp_path)
    for k in ("label_smoothing", "loss_class_weights", "loss_class_weight_power", "loss_positions_from"):
        cfg.pop(k)
    record.clear()
    m, _ = main.run(dict(cfg), data, log=lines.append)
    assert not any("LOSS OBJECTIVE" in l for l in lines) and m.loss_spec is None
