"""mmt_rolling_step on the GPU under teacher forcing: B*S sequences share their first p tokens, one forward over
the B prompts' p tokens fills the workspace, then for every m' = 1..m one mmt_rolling_step(p, m') recomputes each
path's own m' rows and returns the logits at position p + m' - 1. They are compared with the full forward over the
B*S sequences and with the CPU oracle under the three criteria of test_gpu_decode_fanout.py. The step keeps no
state (any order of m' gives the same bits), leaves the workspace alone and refuses before any launch.
"""
import pytest
import torch

import config_utils
import mmt_lib as ML

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -77.0
V3, CROSS3 = [37, 5, 11], [True, False, False]
FACTOR = 2.0  # per position at most twice the full forward's own worst deviation from the oracle


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
    T = meta["block_size"]
    for k in meta["state_dict_keys"]:
        if k.endswith("tril"):
            full[k] = torch.tril(torch.ones(T, T))
    m.load_state_dict(full, strict=True)
    return m


def _model(hs, H, L, T, B, seed):
    """3 modalities, cross-attention on modality 0, perturbed biases and LayerNorms."""
    import mmt_oracle as O
    C = H * hs
    cfg = O.OracleConfig(C, H, L, T, V3, CROSS3)
    g = torch.Generator().manual_seed(seed)
    sd = O.init_params(cfg, g)
    for k in sd:
        if k.endswith("bias") or "ln" in k or "norm" in k:
            sd[k] = sd[k] + 0.05 * torch.randn(sd[k].shape, generator=g)
    tril = [f"blocks.{l}.{kind}.{i}.heads.{h}.tril" for l in range(L) for i in range(len(V3))
            for kind in ("sa_layers", "cross_attention_layers") for h in range(H)
            if kind == "sa_layers" or CROSS3[i]]
    meta = {"n_embd": C, "n_head": H, "n_layer": L, "block_size": T, "B": B, "V": V3, "cross": CROSS3,
            "state_dict_keys": list(sd.keys()) + tril}
    m = build(meta, sd)
    m.eval()
    idx = [torch.randint(0, v, (B, T), generator=g) for v in V3]
    return m, sd, cfg, idx, g


def _paths(idx, S, p, g):
    """[B*S, T] per modality: row b*S + s shares prompt b's first p tokens and has its own after."""
    rows = [t.repeat_interleave(S, 0) for t in idx]
    for i, r in enumerate(rows):
        r[:, p:] = torch.randint(0, V3[i], r[:, p:].shape, generator=g)
    return rows


# name: hs, H, L, T, B, S, p, m
ENGINE_CASES = {
    "c256_hs32": (32, 8, 1, 48, 2, 17, 40, 8),
    "rows_above_a_gemm_tile": (16, 2, 1, 16, 2, 70, 11, 5),
    "one_path_two_layers": (32, 2, 2, 40, 1, 1, 7, 33),
    "hs64_long_prefix": (64, 1, 1, 96, 1, 5, 70, 26),
}


def _check_logits(name, steps, full, ref, p, m, T):
    """steps[m' - 1][i]: [R, V_i], the logits at position p + m' - 1."""
    for i in range(len(V3)):
        got = torch.stack([d[i] for d in steps], dim=1)  # [R, m, V]
        r_full, r_ref = rel(got, full[i][:, p:p + m]), rel(got, ref[i][:, p:p + m])
        e_full = max(rel(full[i][:, t], ref[i][:, t]) for t in range(T))
        per = [rel(steps[t - p][i], ref[i][:, t]) for t in range(p, p + m)]
        e_dec = max(per)
        t_worst = p + per.index(e_dec)
        print(f"rolling engine, {name}, modality {i}: stacked rel vs full {r_full:.2e}, vs oracle {r_ref:.2e}; per "
              f"position max rel vs oracle {e_dec:.2e} (t = {t_worst}), full forward's e_full {e_full:.2e}, "
              f"ratio {e_dec / e_full:.2f}")
        assert r_full < 1e-2, (name, i, r_full)
        assert r_ref < 2e-2, (name, i, r_ref)
        assert e_dec <= FACTOR * e_full, (name, i, t_worst, e_dec, e_full)


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_engine_rolling_teacher_forcing(name):
    import mmt_oracle as O
    hs, H, L, T, B, S, p, m = ENGINE_CASES[name]
    mdl, sd, cfg, idx, g = _model(hs, H, L, T, B, seed=3000 + hs + T + B + S)
    rows = _paths(idx, S, p, g)
    seq = [r.cuda() for r in rows]
    with torch.no_grad():
        full, _ = mdl(seq)
        full = [f.cpu() for f in full]
        mdl([t[:, :p].cuda() for t in idx])
        steps = [[d.cpu() for d in mdl._rolling_step(seq, S, p, k)] for k in range(1, m + 1)]
        # no state between calls: the reverse order of m' gives the same bits, and so does a step called twice
        back = {k: [d.cpu() for d in mdl._rolling_step(seq, S, p, k)] for k in range(m, 0, -1)}
    for k in range(1, m + 1):
        for i in range(len(V3)):
            assert torch.equal(steps[k - 1][i], back[k][i]), (name, k, i)
    ref, _ = O.forward(sd, cfg, rows)
    _check_logits(name, steps, full, ref, p, m, T)


def test_engine_rolling_reads_tokens_in_place_with_a_row_stride():
    """idx_ld: the same tokens inside a wider [rows, cap] buffer, behind other columns, give the same bits."""
    hs, H, L, T, B, S, p, m = 32, 2, 2, 40, 2, 5, 30, 6
    mdl, sd, cfg, idx, g = _model(hs, H, L, T, B, seed=92)
    seq = [r.cuda() for r in _paths(idx, S, p, g)]
    wide = [torch.cat([s, torch.full((B * S, 7), 3, dtype=torch.long, device=DEV)], dim=1) for s in seq]
    exact = [s[:, :p + m].contiguous() for s in seq]
    with torch.no_grad():
        mdl([t[:, :p].cuda() for t in idx])
        a = [x.clone() for x in mdl._rolling_step(seq, S, p, m)]
        b = [x.clone() for x in mdl._rolling_step(wide, S, p, m)]
        c = [x.clone() for x in mdl._rolling_step(exact, S, p, m)]
    for i in range(len(V3)):
        assert torch.equal(a[i], b[i]) and torch.equal(a[i], c[i]), i


def test_engine_rolling_leaves_the_workspace_untouched():
    hs, H, L, T, B, S, p, m = 32, 2, 2, 40, 2, 5, 7, 9
    mdl, sd, cfg, idx, g = _model(hs, H, L, T, B, seed=91)
    seq = [r.cuda() for r in _paths(idx, S, p, g)]
    at_p = [t[:, p].cuda() for t in idx]
    with torch.no_grad():
        mdl([t[:, :p].cuda() for t in idx])
        before = [x.clone() for x in mdl._decode_step(at_p, p)]
        for k in range(1, m + 1):
            mdl._rolling_step(seq, S, p, k)
        after = [x.clone() for x in mdl._decode_step(at_p, p)]
    for i in range(len(V3)):
        assert torch.equal(before[i], after[i]), i


def test_engine_step_refusals_leave_the_logits_alone():
    hs, H, L, T, B, S, p, m = 16, 2, 1, 16, 2, 3, 5, 4
    mdl, sd, cfg, idx, g = _model(hs, H, L, T, B, seed=17)
    Lb = ML.lib()
    R, cap = B * S, 2 * T  # wide enough for the longest tail read from column p
    tok = [torch.zeros(R, cap, dtype=torch.long, device=DEV) for _ in V3]
    logits = [torch.full((R, v), SENTINEL, dtype=torch.float32, device=DEV) for v in V3]
    roll = torch.empty(Lb.mmt_rolling_bytes(mdl._ctx, B, S, T - 1), dtype=torch.uint8, device=DEV)
    tails = ML.ptr_array(tok)
    for i, t in enumerate(tok):
        tails[i] = t.data_ptr() + 8 * p

    def step(p=p, m=m, B=B, S=S, ld=cap, ws=None, buf=ML.ptr(roll), idx=tails, out=None):
        ws = mdl._ws if ws is None else ws
        rc = Lb.mmt_rolling_step(mdl._ctx, ML.stream_ptr(), B, S, p, m, idx, ld, ML.ptr(mdl.flat_params),
                                 ML.ptr_array(logits) if out is None else out, ML.ptr(ws), buf)
        torch.cuda.synchronize()
        return rc

    untouched = lambda: all((x == SENTINEL).all() for x in logits)  # noqa: E731
    assert step(ws=roll) == -4 and untouched()  # MMT_ERR_STATE: no forward yet
    with torch.no_grad():
        mdl([t[:, :p].cuda() for t in idx])
    for kw in (dict(p=0), dict(p=-1), dict(m=0), dict(m=-2), dict(p=T - m + 1), dict(p=1, m=T), dict(S=0), dict(S=-1),
               dict(ld=m - 1), dict(buf=None), dict(idx=None), dict(out=ML.ptr_array([None] * 3)), dict(S=1 << 30),
               dict(B=0), dict(B=-1)):
        assert step(**kw) == -1 and untouched(), kw  # MMT_ERR_INVALID
    assert step(B=B + 1) == -4 and untouched()  # not the forward's batch
    assert step() == 0 and not untouched()
    first = [x.clone() for x in logits]
    for x in logits:
        x.fill_(SENTINEL)
    assert step(p=p + m - 1, m=1) == 0 and torch.isfinite(logits[0]).all()  # any valid (p, m), in any order
    assert step(p=1, m=T - 1) == 0 and torch.isfinite(logits[0]).all()  # the longest tail the buffer was sized for
    assert step() == 0 and all(torch.equal(x, y) for x, y in zip(logits, first))  # the same call, the same bits


def test_rolling_bytes_do_not_grow_with_the_layers():
    Lb = ML.lib()
    one = _model(32, 2, 1, 40, 1, seed=5)[0]
    two = _model(32, 2, 2, 40, 1, seed=5)[0]
    for B, S, m in ((1, 1, 1), (2, 17, 8), (1, 512, 16)):
        a, b = Lb.mmt_rolling_bytes(one._ctx, B, S, m), Lb.mmt_rolling_bytes(two._ctx, B, S, m)
        assert a == b and a > 0, (B, S, m, a, b)
    assert Lb.mmt_fanout_bytes(one._ctx, 2, 17, 8) < Lb.mmt_fanout_bytes(two._ctx, 2, 17, 8)
