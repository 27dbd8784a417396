"""Device-side sampling (include/mmt.h: mmt_sample): temperature, top-k, top-p, draws keyed by
(seed, row, position) and the log-probability of what was drawn, one launch for all rows, no sync.

    tok = mmt_sample.sample(logits, temperature=0.8, top_k=50, top_p=0.9, seed=1234, pos=n)
    tok, lp = mmt_sample.sample(logits, ..., return_logprobs=True)

`model.generate(..., temperature=..., top_k=..., top_p=..., seed=...)` runs on `launch` below; `sample` is the
same entry for users with their own decode loop. The rule is stated in include/mmt.h and INTEGRATION.md.
"""
import torch

import mmt_lib as ML

MASK64 = 2 ** 64 - 1


def check_settings(temperature, top_k, top_p):
    """The three settings as the C entry takes them (None: 1.0 / off / off); ValueError for what it would refuse."""
    t = 1.0 if temperature is None else float(temperature)
    k = 0 if top_k is None else int(top_k)
    p = 1.0 if top_p is None else float(top_p)
    if not t >= 0.0:
        raise ValueError(f"temperature must be >= 0 (0 = greedy), got {temperature!r}")
    if k < 0:
        raise ValueError(f"top_k must be >= 0 (0 = off), got {top_k!r}")
    if p != p:
        raise ValueError("top_p must not be NaN")
    return t, k, p


def device_seed(dev):
    """A 64-bit seed from the device generator's seed and Philox offset (the offset is advanced by 4, as the
    dropout seeds of model.py do); torch's CPU generator is never touched."""
    seed, off = 0, 0
    try:
        gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
        seed = int(gen.initial_seed())
        off = int(gen.get_offset())
        gen.set_offset(off + 4)
    except (AttributeError, RuntimeError, IndexError):
        pass
    x = (seed * 0x9E3779B97F4A7C15 + off * 0xBF58476D1CE4E5B9 + 0x53414D50) & MASK64
    x ^= x >> 31
    x = (x * 0x94D049BB133111EB) & MASK64
    return int(x ^ (x >> 29)) & MASK64


def launch(L, stream, batch, V, logits_ptr, row_stride, t, k, p, seed, row0, pos, tok_ptr, tok_stride, compact_ptr,
           lp_ptr, lp_stride):
    """mmt_sample with raw addresses (ints; 0 = absent). Raises MmtError on a non-zero status."""
    rc = L.mmt_sample(stream, batch, V, logits_ptr, row_stride, t, k, p, seed & MASK64, row0, pos, tok_ptr, tok_stride,
                      compact_ptr or None, lp_ptr or None, lp_stride)
    if rc != 0:
        raise ML.MmtError(f"mmt_sample failed (status {rc})")


def sample(logits, *, temperature=1.0, top_k=0, top_p=1.0, seed, pos, row0=0, return_logprobs=False):
    """One token per row of `logits` (fp32 [B, V] on the GPU; rows may be strided, e.g. `full[:, -1, :]` of a
    [B, T, V] tensor, but elements of a row must be contiguous). Returns int64 [B], with return_logprobs also
    fp32 [B]. `pos` is the sequence position being written and `row0` the index of the first row (for callers
    that split a batch): the draw of row b depends on (seed, row0 + b, pos) and on that row's logits alone."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.device.type != "cuda":
        raise ValueError("sample: logits must be an fp32 [B, V] tensor on the GPU")
    B, V = logits.shape
    if V < 1 or (V > 1 and logits.stride(1) != 1) or (B > 1 and logits.stride(0) < V):
        raise ValueError("sample: the elements of a row must be contiguous and rows must not overlap")
    t, k, p = check_settings(temperature, top_k, top_p)
    dev = logits.device
    tok = torch.empty(B, dtype=torch.int64, device=dev)
    lp = torch.empty(B, dtype=torch.float32, device=dev) if return_logprobs else None
    with torch.cuda.device(dev):
        launch(ML.lib(), ML.stream_ptr(dev), B, V, logits.data_ptr(), max(int(logits.stride(0)), V) if B > 1 else V,
               t, k, p, int(seed), int(row0), int(pos), tok.data_ptr(), 1, 0, lp.data_ptr() if lp is not None else 0, 1)
    return (tok, lp) if return_logprobs else tok
