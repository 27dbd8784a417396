"""The engine's launch structure (csrc/mmt_engine.hip): how many launches each probe label sees in one training
step and in one decode step, through mmt_probe_set / mmt_probe_read_at.

The tables pin which kernels a step launches for whoever fuses two of them next: a fusion changes a row here on
purpose, anything else that changes one is a launch that went missing or came twice. A merged weight-gradient
launch "a+b" counts once, under the first of its parts that matches a pattern. Launches without a label in the
wrapper (LayerNorm passes, keep-bit masks, the decode attention, copies) are not counted.
"""
import ctypes

import pytest
import torch

import config_utils
import mmt_lib as ML
from golden_io import model_fixture

pytestmark = pytest.mark.gpu

LABELS = ["qkv1", "attn_fwd", "proj", "proj0", "proj2", "ffn", "ffn0", "ffn2", "ca_q", "ca_kv", "ca_attn_fwd", "ca_proj",
          "ca_proj0", "ca_proj2", "head0", "head2",
          "head2_dw", "head2_dx", "head0_dw", "head0_dx", "ca_proj2_dw", "ca_proj_dx", "ca_proj2_dx", "ca_proj0_dw",
          "ca_proj0_dx", "ca_attn_bwd", "ca_q_dw", "ca_q_dx", "ca_kv_dw", "ca_kv_dx", "ffn2_dw", "ffn2_dx", "ffn0_dw",
          "ffn0_dx", "proj2_dw", "proj_dx", "proj2_dx", "proj0_dw", "proj0_dx", "attn_bwd", "qkv1_dw", "qkv1_dx",
          "det_sum",
          "dec_qkv1", "dec_proj0", "dec_proj2", "dec_ffn0", "dec_ffn2", "dec_ca_q", "dec_ca_kv", "dec_ca_proj0",
          "dec_ca_proj2", "dec_head0", "dec_head2"]

# Recorded from the build of the commit before the engine's launch wrapper and descriptor builders were unified
# (one forward + backward, deterministic mode off, dropout 0.1; labels with no launch left out). The same file
# passes on that commit unchanged.
TRAIN = {
    "f_small": {"qkv1": 2, "attn_fwd": 2, "proj0": 2, "proj2": 2, "ffn0": 2, "ffn2": 2, "ca_q": 2, "ca_kv": 2,
                "ca_attn_fwd": 2, "ca_proj0": 2, "ca_proj2": 2, "head0": 1, "head2": 1, "head2_dw": 1, "head2_dx": 1,
                "head0_dx": 1, "ca_proj2_dw": 2, "ca_proj2_dx": 2, "ca_proj0_dx": 2, "ca_attn_bwd": 2, "ca_q_dw": 2,
                "ca_q_dx": 2, "ca_kv_dx": 4, "ffn2_dw": 2, "ffn2_dx": 2, "ffn0_dx": 2, "proj2_dw": 2, "proj2_dx": 2,
                "proj0_dx": 2, "attn_bwd": 2, "qkv1_dw": 2, "qkv1_dx": 2},
    "f_hs32": {"qkv1": 1, "attn_fwd": 1, "proj0": 1, "proj2": 1, "ffn0": 1, "ffn2": 1, "ca_q": 1, "ca_kv": 1,
               "ca_attn_fwd": 1, "ca_proj0": 1, "ca_proj2": 1, "head0": 1, "head2": 1, "head2_dw": 1, "head2_dx": 1,
               "head0_dx": 1, "ca_proj2_dw": 1, "ca_proj2_dx": 1, "ca_proj0_dx": 1, "ca_attn_bwd": 1, "ca_q_dw": 1,
               "ca_q_dx": 1, "ca_kv_dx": 1, "ffn2_dw": 1, "ffn2_dx": 1, "ffn0_dx": 1, "proj2_dw": 1, "proj2_dx": 1,
               "proj0_dx": 1, "attn_bwd": 1, "qkv1_dw": 1, "qkv1_dx": 1},
}
# ... and one mmt_decode_step at the last position after an eval-mode prefill
DECODE = {
    "f_small": {"dec_qkv1": 2, "dec_proj0": 2, "dec_proj2": 2, "dec_ffn0": 2, "dec_ffn2": 2, "dec_ca_q": 2,
                "dec_ca_kv": 2, "dec_ca_proj0": 2, "dec_ca_proj2": 2, "dec_head0": 1, "dec_head2": 1},
    "f_hs32": {"dec_qkv1": 1, "dec_proj0": 1, "dec_proj2": 1, "dec_ffn0": 1, "dec_ffn2": 1, "dec_ca_q": 1,
               "dec_ca_kv": 1, "dec_ca_proj0": 1, "dec_ca_proj2": 1, "dec_head0": 1, "dec_head2": 1},
}


def _build(name, dropout, train):
    z, meta, cfg, sd, idx, tgt = model_fixture(name)
    config_utils._config_cache = {"n_embd": meta["n_embd"], "n_head": meta["n_head"], "n_layer": meta["n_layer"],
                                  "block_size": meta["block_size"], "dropout": dropout, "device": "cuda",
                                  "batch_size": meta["B"], "eval_iters": 1, "precision": "bf16"}
    import model as mmt_model
    m = mmt_model.MultimodalTransformer(len(meta["V"]), meta["V"],
                                        [[None] * 8 + [c] + [None] * 3 for c in meta["cross"]]).to("cuda")
    full = {k: t for k, t in m.state_dict().items() if k.endswith("tril")}
    full.update(sd)
    m.load_state_dict(full, strict=True)
    m._next_dropout_seed = lambda dev: 0x5EED1234
    m.train(train)
    m.set_deterministic(False)
    return m, [t.cuda() for t in idx], [t.cuda() for t in tgt]


def _counts(m, step):
    """{label: launches} of step(), labels without a launch left out."""
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
            if n.value:
                out[lab] = n.value
        return out
    finally:
        L.mmt_probe_set(m._ctx, None)


@pytest.mark.parametrize("name", ["f_small", "f_hs32"])
def test_training_step_launches(name):
    m, idx, tgt = _build(name, 0.1, True)

    def step():
        m.flat_params.grad = None
        _, losses = m(idx, tgt)
        sum(losses).backward()

    got = _counts(m, step)
    print(f"{name} training step: {got}")
    assert got == TRAIN[name]


@pytest.mark.parametrize("name", ["f_small", "f_hs32"])
def test_decode_step_launches(name):
    m, idx, _ = _build(name, 0.0, False)
    T = idx[0].shape[1]
    with torch.no_grad():
        m(idx)  # the prefill
        got = _counts(m, lambda: m._decode_step([t[:, -1] for t in idx], T - 1))
    print(f"{name} decode step: {got}")
    assert got == DECODE[name]
