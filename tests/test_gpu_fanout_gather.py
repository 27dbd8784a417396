"""mmt_fanout_gather (csrc/mmt_engine.hip, the gather kernel in csrc/mmt_evidence.hip) on the f_small fixture (d64, L2,
T32, V = [57, 13, 24, 5], cross-attention on modalities 0 and 2): after five fan-out steps the tails of a NaN-filled
second buffer must hold, for the copied positions, the keys and values of each row's ancestor, bit for bit.

The tails lie at the end of the fan buffer in plan order (include/mmt.h mmt_fanout_bytes): per (layer, modality)
the self-attention tail [R, N, 3C], columns K | Q | V, then for a cross modality one [R, N, 2C] tail per KV stream,
each rounded up to 256 bytes."""
import numpy as np
import pytest
import torch

import mmt_lib as ML
from golden_io import model_fixture
from test_gpu_generate_device import build

pytestmark = pytest.mark.gpu

B, N0, N, STEPS = 2, 8, 12, 5
NAN16 = 0x7FC0  # the bf16 quiet NaN


@pytest.fixture(scope="module")
def small():
    z, meta, cfg, sd, idx, tgt = model_fixture("f_small")
    m = build(meta, sd)
    m.eval()
    return meta, idx, m


def tails(meta, R, total):
    """[(byte offset, ld, key/value columns)] of every tail, and the offset of the first."""
    C, M = meta["n_embd"], len(meta["V"])
    rup = lambda x: -(-x // 256) * 256  # noqa: E731
    sizes = []
    for _ in range(meta["n_layer"]):
        for i in range(M):
            sizes.append((rup(R * N * 3 * C * 2), 3 * C, list(range(C)) + list(range(2 * C, 3 * C))))
            if meta["cross"][i]:
                sizes += [(rup(R * N * 2 * C * 2), 2 * C, list(range(2 * C)))] * (M - 1)
    off = total - sum(s[0] for s in sizes)
    first, out = off, []
    for nbytes, ld, cols in sizes:
        out.append((off, ld, cols))
        off += nbytes
    return out, first


def ancestors(S, kind):
    a = np.arange(B * S, dtype=np.int32)
    if kind == "mixed":
        a[:S] = (np.arange(S) // 3) * 3  # prompt 0: duplicates (and rows that die)
        a[S:] = S + np.arange(S)[::-1]  # prompt 1: a reversal
    return a


def run_steps(m, meta, idx, S):
    """Prefill over B prompts and STEPS fan-out steps with random tokens; returns the run's fan buffer."""
    g = torch.Generator().manual_seed(11 + S)
    with torch.no_grad():
        m([t[:B, :N0].cuda() for t in idx])
        for k in range(STEPS):
            tok = [torch.randint(0, v, (B * S,), generator=g).cuda() for v in meta["V"]]
            m._decode_fanout_step(tok, N0 + k, S, N0, N)
    torch.cuda.synchronize()
    return m._fan


def gather(m, S, anc, src, dst, npos=STEPS, shape=None):
    a = dict(B=B, S=S, n0=N0, N=N)
    a.update(shape or {})
    rc = ML.lib().mmt_fanout_gather(m._ctx, ML.stream_ptr(), a["B"], a["S"], a["n0"], a["N"], npos, ML.ptr(anc),
                                    ML.ptr(src), ML.ptr(dst))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("S", [8, 17])
@pytest.mark.parametrize("kind", ["mixed", "identity"])
def test_gather_moves_keys_and_values_to_their_ancestors(small, S, kind):
    meta, idx, m = small
    R = B * S
    src = run_steps(m, meta, idx, S)
    before = src.clone()
    dst = torch.empty_like(src)
    dst.view(torch.int16).fill_(NAN16)
    anc = ancestors(S, kind)
    assert gather(m, S, torch.from_numpy(anc).cuda(), src, dst) == 0
    assert torch.equal(src, before), "the source changed"
    segs, first = tails(meta, R, src.numel())
    assert bool((dst[:first].view(torch.int16) == NAN16).all()), "the per-step scratch was written"
    s16, d16 = src.cpu().view(torch.int16), dst.cpu().view(torch.int16)
    for off, ld, cols in segs:
        s = s16[off // 2: off // 2 + R * N * ld].view(R, N, ld)[:, :STEPS][:, :, cols]
        d = d16[off // 2: off // 2 + R * N * ld].view(R, N, ld)[:, :STEPS][:, :, cols]
        assert not bool((s == NAN16).all(-1).any()), "the run left a copied position unwritten"
        assert torch.equal(d, s[torch.from_numpy(anc).long()]), (off, ld)
    # the next step runs from dst and gives finite logits
    tok = [torch.zeros(R, dtype=torch.long, device="cuda") for _ in meta["V"]]
    logits = [torch.full((R, v), float("nan"), dtype=torch.float32, device="cuda") for v in meta["V"]]
    rc = ML.lib().mmt_decode_fanout_step(m._ctx, ML.stream_ptr(), B, S, N0, N, N0 + STEPS, ML.ptr_array(tok),
                                         ML.ptr(m.flat_params), ML.ptr_array(logits), ML.ptr(m._ws), ML.ptr(dst))
    torch.cuda.synchronize()
    assert rc == 0
    assert all(bool(torch.isfinite(x).all()) for x in logits)
    if kind == "mixed":  # rows of one ancestor and one token see one history (1e-2: the decode-vs-forward bound)
        for r in (1, 2):
            assert ((logits[0][r] - logits[0][0]).norm() / logits[0][0].norm()).item() < 1e-2, r


def test_gather_refuses_before_any_write(small):
    meta, idx, m = small
    S = 8
    src = run_steps(m, meta, idx, S)
    dst = torch.empty_like(src)
    dst.view(torch.int16).fill_(NAN16)
    anc = torch.from_numpy(ancestors(S, "mixed")).cuda()
    untouched = lambda: bool((dst.view(torch.int16) == NAN16).all())  # noqa: E731
    assert gather(m, S, anc, src, src) == -1 and untouched()  # src == dst
    for kw in (dict(S=S + 1), dict(B=B + 1), dict(n0=N0 + 1), dict(N=N - 1)):
        assert gather(m, S, anc, src, dst, shape=kw) == -4 and untouched(), kw  # not the run in progress
    for npos in (STEPS - 1, STEPS + 1, 0):
        assert gather(m, S, anc, src, dst, npos=npos) == -1 and untouched(), npos
    assert gather(m, S, None, src, dst) == -1 and untouched()
    assert gather(m, S, anc, None, dst) == -1 and untouched()
    assert gather(m, S, anc, src, None) == -1
    with torch.no_grad():
        m([t[:B, :N0].cuda() for t in idx])  # a new prefill ends the run
    assert gather(m, S, anc, src, dst) == -4 and untouched()
