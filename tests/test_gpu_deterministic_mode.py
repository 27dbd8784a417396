"""Deterministic training mode (mmt_set_deterministic, include/mmt.h): bitwise-reproducible gradients and runs.

tests/test_gpu_determinism.py states what the default mode gives: a bitwise repeatable forward and a
gradient repeatable to a rel-L2 of GRAD_BOUND, because the bias / LayerNorm / stage-2 / embedding column
sums leave their kernels as one float atomic per block and add in arrival order. With the mode on those
sums leave as per-block partials and one ordered sum adds them, so everything here is compared with
torch.equal. Every model is built as that file builds it: dropout 0.1, the mask seed pinned.

A failing bitwise check prints, per reference tensor, how many entries differ, so the red test names the
kernel site (a bias -> a GEMM epilogue's column sums, ln*.weight -> the LayerNorm backward, ...).
"""
import ctypes
import functools
import random

import pytest
import torch

import config_utils
import mmt_lib as ML
from golden_io import model_fixture, scale_fixture

pytestmark = pytest.mark.gpu

# the project's bound for "same sums, different order" (tests/test_gpu_determinism.py)
GRAD_BOUND = 1e-6
PINNED_SEED = 0x5EED1234


class Case:
    def __init__(self, name, C, H, L, T, V, cross, B, sd, idx, tgt, precision="bf16", z=None, meta=None):
        self.name, self.C, self.H, self.L, self.T, self.V, self.cross, self.B = name, C, H, L, T, V, cross, B
        self.sd, self.idx, self.tgt, self.precision, self.z, self.meta = sd, idx, tgt, precision, z, meta


@functools.lru_cache(maxsize=None)
def _case(name):
    """The shapes of the issue's table; parameters, inputs (and the golden gradient) made once and shared."""
    if name in ("o_c512", "o_c40"):
        import mmt_oracle as O
        if name == "o_c512":  # 128 x 512 row-wide tile, mlp2_bwd at 512, R = 192 ragged against the row tiles
            C, H, L, T, B, V, cross, seed = 512, 8, 1, 64, 3, [11, 7], [True, False], 5
        else:  # the shape of test_relu_bits_ragged_hidden_width: the scalar edge epilogue
            C, H, L, T, B, V, cross, seed = 40, 5, 2, 16, 3, [11, 7], [True, False], 11
        g = torch.Generator().manual_seed(seed)
        sd = O.init_params(O.OracleConfig(C, H, L, T, V, cross), g)
        idx = [torch.randint(0, v, (B, T), generator=g) for v in V]
        tgt = [torch.randint(0, v, (B, T), generator=g) for v in V]
        return Case(name, C, H, L, T, V, cross, B, sd, idx, tgt)
    fx, _, prec = name.partition(":")
    z, meta, cfg, sd, idx, tgt = (scale_fixture if fx in ("f_c1", "f_m8", "f_t1024") else model_fixture)(fx)
    return Case(name, meta["n_embd"], meta["n_head"], meta["n_layer"], meta["block_size"], meta["V"], meta["cross"],
                meta["B"], sd, idx, tgt, prec or "bf16", z, meta)


def _build(case, det, dropout=0.1):
    config_utils._config_cache = {"n_embd": case.C, "n_head": case.H, "n_layer": case.L, "block_size": case.T,
                                  "dropout": dropout, "device": "cuda", "batch_size": case.B, "eval_iters": 1,
                                  "precision": case.precision}
    import model as mmt_model
    m = mmt_model.MultimodalTransformer(len(case.V), case.V, [[None] * 8 + [c] + [None] * 3 for c in case.cross]).to("cuda")
    full = {k: t for k, t in m.state_dict().items() if k.endswith("tril")}
    full.update(case.sd)
    m.load_state_dict(full, strict=True)
    m._next_dropout_seed = lambda dev: PINNED_SEED  # the same masks on every forward
    m.train()
    m.set_deterministic(det)
    return m


def _data(case):
    return [t.cuda() for t in case.idx], [t.cuda() for t in case.tgt]


def _fwd_bwd(m, idx, tgt):
    m.flat_params.grad = None
    logits, losses = m(idx, tgt)
    sum(losses).backward()
    torch.cuda.synchronize()
    return ([l.detach().clone() for l in logits], torch.stack([l.detach() for l in losses]).clone(),
            m.flat_params.grad.detach().clone())


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _mismatch_report(m, ga, gb):
    """Per reference tensor: entries of the two flat gradients that differ (names the kernel site)."""
    lines = []
    for name, off, shp, _ in m._tensors:
        n = 1
        for s in shp:
            n *= s
        if off >= m._n_active:
            continue
        d = int((ga[off:off + n] != gb[off:off + n]).sum().item())
        if d:
            lines.append(f"  {name}: {d} of {n} entries differ")
    # (the same slices reference_grad_views() hands out)
    assert [k for k, _ in m.reference_grad_views()] == [t[0] for t in m._tensors]
    return "\n".join(lines) or "  (no tensor differs)"


def _assert_same_bits(m, out_a, out_b, what):
    (lg_a, ls_a, g_a), (lg_b, ls_b, g_b) = out_a, out_b
    assert torch.equal(ls_a, ls_b), (what, ls_a, ls_b)
    for a, b in zip(lg_a, lg_b):
        assert torch.equal(a, b), what
    if not torch.equal(g_a, g_b):
        rep = _mismatch_report(m, g_a, g_b)
        print(f"{what}: gradients differ\n{rep}")
        pytest.fail(f"{what}: gradients are not bitwise equal (rel-L2 {_rel(g_a, g_b):.3e})\n{rep}")


# ------------------------------------------------------------------------------------------------
# 1. two (three) backward passes: bitwise equal gradients, logits and losses
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,passes", [("f_small", 3), ("f_hs32", 2), ("f_c1", 3), ("f_m8:bf16", 2), ("f_m8:fp8", 2),
                                         ("f_t1024", 2), ("o_c512", 2), ("o_c40", 2)])
def test_backward_twice_same_bits(name, passes):
    case = _case(name)
    m = _build(case, True)
    assert m.deterministic is True
    idx, tgt = _data(case)
    first = _fwd_bwd(m, idx, tgt)
    assert torch.isfinite(first[2]).all() and first[2].abs().max() > 0
    for k in range(1, passes):
        _assert_same_bits(m, _fwd_bwd(m, idx, tgt), first, f"{name} pass {k + 1} vs pass 1")


# ------------------------------------------------------------------------------------------------
# 2. the same math as the default mode
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f_small", "f_c1", "f_m8:bf16"])
def test_same_math_as_default_mode(name):
    case = _case(name)
    idx, tgt = _data(case)
    lg_d, ls_d, g_d = _fwd_bwd(_build(case, True), idx, tgt)
    lg_0, ls_0, g_0 = _fwd_bwd(_build(case, False), idx, tgt)
    assert torch.equal(ls_d, ls_0)
    for a, b in zip(lg_d, lg_0):
        assert torch.equal(a, b)  # the forward does not depend on the mode
    err = _rel(g_d, g_0)
    print(f"{name}: deterministic vs default gradient rel-L2 {err:.3e}")
    assert err <= GRAD_BOUND, err


def test_matches_golden_gradient():
    """f_small without dropout against the reference's recorded gradient, at the bf16 tolerance
    test_relu_bits_match_bf16_aux uses."""
    case = _case("f_small")
    idx, tgt = _data(case)
    m = _build(case, True, dropout=0.0)
    _fwd_bwd(m, idx, tgt)
    grads = dict(m.reference_grad_views())
    none = set(case.meta["grad_none"])
    a = torch.cat([g.flatten().cpu() for k, g in grads.items() if k not in none])
    b = torch.cat([torch.from_numpy(case.z[f"grad.{k}"]).flatten() for k in grads if k not in none])
    err = _rel(a, b)
    print(f"f_small deterministic vs golden gradient rel-L2 {err:.3e}")
    assert err < 3e-2, err


# ------------------------------------------------------------------------------------------------
# 3. a short run replays
# ------------------------------------------------------------------------------------------------
def _short_run(case, steps=8):
    import mmt_optim
    torch.manual_seed(1234)
    random.seed(1234)
    m = _build(case, True)
    opt = mmt_optim.AdamW(m.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(99)
    batches = [([torch.randint(0, v, (case.B, case.T), generator=g).cuda() for v in case.V],
                [torch.randint(0, v, (case.B, case.T), generator=g).cuda() for v in case.V]) for _ in range(steps)]
    hist = []
    for idx, tgt in batches:
        _, losses = m(idx, tgt)
        opt.zero_grad(set_to_none=True)
        sum(losses).backward()
        opt.step()
        hist.append(torch.stack([l.detach() for l in losses]).clone())
    torch.cuda.synchronize()
    return torch.stack(hist).cpu(), m.flat_params.detach().clone().cpu()


@pytest.mark.parametrize("name", ["f_small", "f_c1"])
def test_short_run_replays(name):
    case = _case(name)
    h1, p1 = _short_run(case)
    h2, p2 = _short_run(case)
    assert torch.isfinite(h1).all() and not torch.equal(h1[0], h1[-1])
    diff_steps = [s for s in range(h1.shape[0]) if not torch.equal(h1[s], h2[s])]
    assert not diff_steps, f"losses differ at steps {diff_steps}: {h1[diff_steps[0]]} vs {h2[diff_steps[0]]}"
    assert torch.equal(p1, p2), f"{int((p1 != p2).sum())} of {p1.numel()} parameters differ after 8 steps"


# ------------------------------------------------------------------------------------------------
# 4. the ordered-sum primitive
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nparts", [1, 2, 7, 64, 257])
@pytest.mark.parametrize("n", [1, 5, 256, 1000])
def test_ordered_sum_primitive(nparts, n):
    """dst += ((p0 + p1) + p2) + ... in index order, fp32: bitwise the same chain of CPU tensor adds. 257
    partials spanning several exponents: a pairwise tree or an FMA would round differently."""
    L = ML.lib()
    ld = n + 3
    g = torch.Generator().manual_seed(1000 * nparts + n)
    parts = torch.randn(nparts, ld, generator=g) * torch.pow(2.0, torch.randint(-12, 13, (nparts, ld), generator=g).float())
    dst0 = torch.randn(n, generator=g)
    acc = parts[0, :n].clone()
    for k in range(1, nparts):
        acc = acc + parts[k, :n]
    want = dst0 + acc
    pd, dd = parts.cuda(), dst0.cuda()
    guard = pd.clone()
    ML.check(L.mmt_op_ordered_sum(ML.stream_ptr(), nparts, n, ML.ptr(pd), ld, ML.ptr(dd)), None, "mmt_op_ordered_sum")
    torch.cuda.synchronize()
    assert torch.equal(dd.cpu(), want), int((dd.cpu() != want).sum())
    assert torch.equal(pd, guard)  # the partials (and their pad columns) are only read
    if nparts == 257 and n == 1000:  # the case is sharp: a pairwise tree gives other bits somewhere
        tree = [parts[k, :n] for k in range(nparts)]
        while len(tree) > 1:
            tree = [tree[i] + tree[i + 1] if i + 1 < len(tree) else tree[i] for i in range(0, len(tree), 2)]
        assert not torch.equal(dst0 + tree[0], want)


# ------------------------------------------------------------------------------------------------
# 5. stale scratch
# ------------------------------------------------------------------------------------------------
def test_small_shape_after_large_shape_reads_no_stale_partials():
    """f_c1 first, then f_small, on models sharing nothing but the process (the caching allocator hands the
    second workspace memory the first one wrote); then f_small alone in a fresh model: the same bits. A sum
    over partial rows its launch did not write would differ."""
    big, small = _case("f_c1"), _case("f_small")
    mb = _build(big, True)
    _fwd_bwd(mb, *_data(big))
    del mb
    ms = _build(small, True)
    idx, tgt = _data(small)
    after_big = _fwd_bwd(ms, idx, tgt)
    del ms
    torch.cuda.empty_cache()
    m = _build(small, True)
    alone = _fwd_bwd(m, idx, tgt)
    _assert_same_bits(m, after_big, alone, "f_small after f_c1 vs f_small alone")


# ------------------------------------------------------------------------------------------------
# 6. switch semantics
# ------------------------------------------------------------------------------------------------
def test_getter_reflects_setter():
    case = _case("f_small")
    m = _build(case, False)
    L = ML.lib()
    assert m.deterministic is False and L.mmt_get_deterministic(m._ctx) == 0
    m.set_deterministic(True)
    assert m.deterministic is True and L.mmt_get_deterministic(m._ctx) == 1
    m.set_deterministic(False)
    assert m.deterministic is False and L.mmt_get_deterministic(m._ctx) == 0
    config_utils._config_cache = dict(config_utils._config_cache, deterministic=True)
    import model as mmt_model
    m2 = mmt_model.MultimodalTransformer(len(case.V), case.V, [[None] * 8 + [c] + [None] * 3 for c in case.cross])
    assert m2.deterministic is True and L.mmt_get_deterministic(m2._ctx) == 1


def test_toggle_between_forward_and_backward_does_not_affect_that_backward():
    """Latched by the forward: a forward under the mode, the switch turned off, then the backward, gives the
    bits of an undisturbed deterministic step (and keeps giving them)."""
    case = _case("f_small")
    idx, tgt = _data(case)
    m = _build(case, True)
    ref = _fwd_bwd(m, idx, tgt)
    for _ in range(2):
        m.set_deterministic(True)
        m.flat_params.grad = None
        logits, losses = m(idx, tgt)
        m.set_deterministic(False)  # requested, applied by the NEXT forward only
        sum(losses).backward()
        torch.cuda.synchronize()
        got = ([l.detach().clone() for l in logits], torch.stack([l.detach() for l in losses]).clone(),
               m.flat_params.grad.detach().clone())
        _assert_same_bits(m, got, ref, "backward after toggling the switch off")


def test_mode_off_after_on_is_the_default_mode():
    case = _case("f_small")
    idx, tgt = _data(case)
    never = _fwd_bwd(_build(case, False), idx, tgt)
    m = _build(case, True)
    _fwd_bwd(m, idx, tgt)
    m.set_deterministic(False)
    lg, ls, g = _fwd_bwd(m, idx, tgt)
    assert torch.equal(ls, never[1])
    for a, b in zip(lg, never[0]):
        assert torch.equal(a, b)
    assert _rel(g, never[2]) <= GRAD_BOUND, _rel(g, never[2])


# ------------------------------------------------------------------------------------------------
# 7. the embedding limit
# ------------------------------------------------------------------------------------------------
def test_embedding_limit_is_refused_not_run_in_arrival_order():
    """B * T = 513 * 32 > 16384 rows: past the stable row sort, so in the mode the backward returns
    MMT_ERR_UNSUPPORTED naming the limit before launching anything (the gradient buffer is untouched); the
    default mode runs as before."""
    C, H, L_, T, V, B = 32, 2, 1, 32, [5], 513
    config_utils._config_cache = {"n_embd": C, "n_head": H, "n_layer": L_, "block_size": T, "dropout": 0.1,
                                  "device": "cuda", "batch_size": B, "eval_iters": 1}
    import model as mmt_model
    torch.manual_seed(3)
    m = mmt_model.MultimodalTransformer(1, V, [[None] * 8 + [False] + [None] * 3]).to("cuda")
    m._next_dropout_seed = lambda dev: PINNED_SEED
    m.train()
    g = torch.Generator().manual_seed(4)
    idx = [torch.randint(0, V[0], (B, T), generator=g).cuda()]
    tgt = [torch.randint(0, V[0], (B, T), generator=g).cuda()]
    # default mode: runs
    _, _, g0 = _fwd_bwd(m, idx, tgt)
    assert torch.isfinite(g0).all() and g0.abs().max() > 0
    # deterministic mode: refused at stage 0, nothing launched
    m.set_deterministic(True)
    m.flat_params.grad = None
    _, losses = m(idx, tgt)
    L = ML.lib()
    grads = torch.full((m._n_active,), 7.0, device="cuda")
    lg = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    rc = L.mmt_backward(m._ctx, ML.stream_ptr(), ML.ptr(lg), ML.ptr(m.flat_params.data), ML.ptr(grads), ML.ptr(m._ws))
    torch.cuda.synchronize()
    assert rc == -2, rc  # MMT_ERR_UNSUPPORTED
    msg = L.mmt_last_error(m._ctx).decode()
    assert "16384" in msg and "deterministic" in msg, msg
    assert bool((grads == 7.0).all()), "the refused backward wrote into the gradient buffer"
    with pytest.raises(ML.MmtError, match="16384"):
        sum(losses).backward()
    # and the default mode again afterwards
    m.set_deterministic(False)
    _, _, g1 = _fwd_bwd(m, idx, tgt)
    assert _rel(g1, g0) <= GRAD_BOUND
