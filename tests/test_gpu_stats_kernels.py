"""Kernel-level checks of mmt_tensor_stats (include/mmt.h) on synthetic buffers against an fp64 restatement
in numpy: every size at which the kernels change path, exactness, gaps and guard bands, non-finite values at
the awkward places, bit-reproducibility, the first-skipped-step latch, invalid arguments, no host sync.

Buffer A (8 chunks of STATS_CHUNK, n not a multiple of 4) is laid out so that one call meets: segments of 1,
3, 4 and 5 elements, an empty one, one that begins and ends off a 4-boundary, 300 segments of 1-16 elements
inside one chunk (lanes that hold up to four runs, runs closed at every level of the wave tree), a segment of
exactly one chunk (all four waves on the streaming path), one that straddles two chunks, one over four chunks,
gaps before the first, between and after the last segment, and the buffer's partial last vector. Buffer B is
one segment over 301 chunks: more chunk partials than the 64 lanes of its second-pass wave.

Bounds. absmax, the counts and first_bad are exact. sqsum: each fp32 square is exact in fp64 and every term is
non-negative, so any summation order of k terms is within (k - 1) * 2^-53 relative of the exact sum; the
reference is math.fsum (correctly rounded: 2^-53), together k * 2^-53.
"""
import functools
import math

import numpy as np
import pytest
import torch

import mmt_lib as ML
import mmt_optim
import mmt_stats

pytestmark = pytest.mark.gpu

CH = ML.STATS_CHUNK
U = 2.0 ** -53
BAND = 256
PATTERN = 0xA5
B1, B2 = 0.9, 0.999


def _stream():
    return ML.stream_ptr(torch.device("cuda"))


# ------------------------------------------------------------------------------------------------ layouts
@functools.lru_cache(maxsize=None)
def _layout_a():
    """names, begins, ends, n of buffer A; made once, never modified."""
    rng = np.random.default_rng(11)
    segs = [("one", 3, 4), ("three", 4, 7), ("four", 9, 13), ("five", 13, 18), ("empty", 18, 18),
            ("odd", 21, 1030)]
    at = 1031
    for i, ln in enumerate(rng.integers(1, 17, size=300)):
        if i % 37 == 36:
            at += int(rng.integers(1, 4))  # a few gaps among the small ones
        segs.append((f"small{i}", at, at + int(ln)))
        at += int(ln)
    assert at < CH - 8
    segs += [("chunk", CH, 2 * CH), ("two", 2 * CH + 100, 3 * CH + 200), ("many", 3 * CH + 212, 6 * CH + 289),
             ("tail", 6 * CH + 292, 7 * CH + 118)]
    n = 7 * CH + 123
    names, begins, ends = [s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs]
    return names, begins, ends, n


@functools.lru_cache(maxsize=None)
def _layout_b():
    n = 301 * CH - 90
    return ["long"], [5], [n - 3], n


@functools.lru_cache(maxsize=None)
def _values(n, seed):
    """fp32 values over many binades (so absmax and the squares are not all alike); never modified."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 6, size=n))).astype(np.float32)
    x.setflags(write=False)
    return x


def _fill(layout, seed, bad=()):
    """The host buffer: values inside the named segments, NaN in every gap, then `bad` = [(index, value)]."""
    names, begins, ends, n = layout
    x = np.full(n, np.nan, dtype=np.float32)
    v = _values(n, seed)
    for b, e in zip(begins, ends):
        x[b:e] = v[b:e]
    for i, val in bad:
        x[i] = val
    return x


def _reference(x, begins, ends):
    """The fp64 restatement: per segment (sqsum, nan, inf, first_bad, absmax)."""
    out = []
    for b, e in zip(begins, ends):
        s = x[b:e]
        fin = np.isfinite(s)
        f64 = s[fin].astype(np.float64)
        bad = np.nonzero(~fin)[0]
        out.append((math.fsum((f64 * f64).tolist()), int(np.isnan(s).sum()), int(np.isinf(s).sum()),
                    int(bad[0]) if len(bad) else -1, float(np.abs(s[fin]).max()) if fin.any() else 0.0))
    return out


class _Call:
    """Device table, record and scratch of one layout, the last two followed by a band of PATTERN bytes."""

    def __init__(self, layout, fill=0):
        names, begins, ends, n = layout
        self.names, self.begins, self.ends, self.n = names, begins, ends, n
        self.bounds, self.named = mmt_stats.build_segments(names, begins, ends)
        self.nseg = len(self.bounds) - 1
        L = ML.lib()
        self.rec_bytes = L.mmt_stats_record_bytes(self.nseg)
        self.scr_bytes = L.mmt_stats_scratch_bytes(n, self.nseg)
        assert self.rec_bytes == 32 + 40 * self.nseg and self.scr_bytes == 32 * ((n + CH - 1) // CH + self.nseg)
        self.table = torch.tensor(self.bounds, dtype=torch.int64).cuda()
        self.rec = torch.full((self.rec_bytes + BAND,), fill, dtype=torch.uint8, device="cuda")
        self.rec[self.rec_bytes:] = PATTERN
        self.scratch = torch.full((self.scr_bytes + BAND,), PATTERN, dtype=torch.uint8, device="cuda")

    def run(self, x, mode=ML.STATS_ALWAYS, guard=None):
        return ML.lib().mmt_tensor_stats(_stream(), ML.ptr(x), x.numel(), ML.ptr(self.table), self.nseg, mode,
                                         ML.ptr(guard), ML.ptr(self.scratch), ML.ptr(self.rec))

    def raw(self):
        torch.cuda.synchronize()
        return self.rec[:self.rec_bytes].cpu().numpy().tobytes()

    def report(self):
        return mmt_stats.StatsReport.from_record(self.raw(), self.names, self.named)

    def bands_intact(self):
        return bool((self.rec[self.rec_bytes:] == PATTERN).all()) and bool((self.scratch[self.scr_bytes:] == PATTERN).all())


def _check(call, x_host, rep):
    ref = _reference(x_host, call.begins, call.ends)
    worst = 0.0
    for i, (name, (sq, nan, inf, fb, amax)) in enumerate(zip(call.names, ref)):
        k = call.ends[i] - call.begins[i]
        got = float(rep.sqsum[i])
        err = abs(got - sq) / sq if sq > 0 else abs(got)
        worst = max(worst, err / (max(k, 1) * U))
        assert err <= k * U, (name, got, sq, err / U, k)
        assert float(rep.absmax[i]) == amax, (name, float(rep.absmax[i]), amax)
        assert (int(rep.nan_count[i]), int(rep.inf_count[i]), int(rep.first_bad[i])) == (nan, inf, fb), name
    return worst


# ------------------------------------------------------------------------------------------------ values
def test_every_path_matches_the_fp64_reference():
    lay = _layout_a()
    x = _fill(lay, 1)  # every gap is NaN: no statistic may see it
    call = _Call(lay)
    assert call.run(torch.from_numpy(x).cuda()) == 0
    rep = call.report()
    hdr = ML.MmtStatsHeader.from_buffer_copy(call.raw()[:32])
    assert (hdr.valid, hdr.nseg, hdr.applied_steps, hdr.skipped_steps, hdr.reserved) == (1, call.nseg, 0, 0, 0)
    worst = _check(call, x, rep)
    print(f"buffer A: {len(call.names)} named of {call.nseg} segments, worst sqsum error {worst:.3f} of its bound")
    assert not rep.nonfinite() and call.bands_intact()
    i = call.names.index("empty")
    assert (rep.sqsum[i], rep.absmax[i], rep.nan_count[i], rep.inf_count[i], rep.first_bad[i]) == (0.0, 0.0, 0, 0, -1)


def test_long_segment_with_more_chunks_than_lanes():
    lay = _layout_b()
    x = _fill(lay, 2)
    call = _Call(lay)
    assert call.run(torch.from_numpy(x).cuda()) == 0
    worst = _check(call, x, call.report())
    print(f"buffer B: {lay[3]} elements in {(lay[3] + CH - 1) // CH} chunks, sqsum error {worst:.2e} of its bound")
    assert call.bands_intact()


def test_nonfinite_values_at_the_awkward_places():
    lay = _layout_a()
    names, begins, ends, n = lay
    at = {nm: (b, e) for nm, b, e in zip(names, begins, ends)}
    nan, inf = float("nan"), float("inf")
    bad = [(at["three"][0], inf), (at["three"][1] - 1, nan),          # a segment's first and last element
           (at["one"][0], -inf),                                      # a one-element segment
           (at["odd"][0], nan), (at["odd"][1] - 1, -inf),             # the unaligned head and tail
           (at["small7"][0], inf), (at["small150"][1] - 1, nan),      # inside the crowded chunk
           (CH, nan), (2 * CH - 1, inf),                              # both sides of chunk boundaries
           (3 * CH - 1, -inf), (3 * CH, nan),                         # a boundary inside the straddling segment
           (4 * CH + 10, inf), (5 * CH + 4000, nan), (5 * CH + 4001, nan),  # the long segment's later chunks
           (n - 6, nan)]                                              # the last element of the last segment
    x = _fill(lay, 3, bad)
    call = _Call(lay)
    assert call.run(torch.from_numpy(x).cuda()) == 0
    rep = call.report()
    _check(call, x, rep)  # counts and first_bad exact, sqsum / absmax over the finite elements only
    hit = {nm for nm, *_ in rep.nonfinite()}
    assert hit == {"three", "one", "odd", "small7", "small150", "chunk", "two", "many", "tail"}
    i = names.index("many")
    assert (int(rep.nan_count[i]), int(rep.inf_count[i]), int(rep.first_bad[i])) == (2, 1, 4 * CH + 10 - begins[i])
    assert call.bands_intact()


def test_two_calls_give_identical_records():
    for lay, seed in ((_layout_a(), 4), (_layout_b(), 5)):
        x = torch.from_numpy(_fill(lay, seed, [(lay[1][-1] + 1, float("inf"))])).cuda()
        one, two = _Call(lay), _Call(lay, fill=0xFF)
        assert one.run(x) == 0 and two.run(x) == 0 and one.run(x) == 0
        torch.cuda.synchronize()
        assert torch.equal(one.rec[:one.rec_bytes], two.rec[:two.rec_bytes])


def test_unsegmented_elements_and_nseg_zero():
    """A table that covers only the middle of the buffer, and no table at all."""
    n = 2 * CH + 9
    x_host = _values(n, 6).copy()
    x_host[:100] = np.nan
    x_host[CH + 50:] = np.inf
    lay = (("mid",), (100,), (CH + 50,), n)
    call = _Call(lay)
    assert call.run(torch.from_numpy(x_host).cuda()) == 0
    _check(call, x_host, call.report())
    rec = torch.full((32 + BAND,), PATTERN, dtype=torch.uint8, device="cuda")
    rc = ML.lib().mmt_tensor_stats(_stream(), ML.ptr(torch.from_numpy(x_host).cuda()), n, ML.ptr(call.table), 0,
                                   ML.STATS_ALWAYS, None, ML.ptr(call.scratch), ML.ptr(rec))
    assert rc == 0
    torch.cuda.synchronize()
    hdr = ML.MmtStatsHeader.from_buffer_copy(rec[:32].cpu().numpy().tobytes())
    assert (hdr.valid, hdr.nseg, hdr.applied_steps, hdr.skipped_steps) == (1, 0, 0, 0)
    assert bool((rec[32:] == PATTERN).all())


# ------------------------------------------------------------------------------------------------ latch
def _guard_for(g, skip=True):
    """A guard state after mmt_grad_sqsum + mmt_guard_finalize on g (the normal way to ok = 0 / 1)."""
    L = ML.lib()
    guard = torch.zeros(L.mmt_guard_state_bytes(), dtype=torch.uint8, device="cuda")
    return guard, lambda grad: (L.mmt_grad_sqsum(_stream(), ML.ptr(grad), grad.numel(), 0, ML.ptr(guard)),
                                L.mmt_guard_finalize(_stream(), 0.0, 1 if skip else 0, B1, B2, ML.ptr(guard)))


def test_latch_keeps_the_first_skipped_step():
    lay = _layout_a()
    names, begins, ends, n = lay
    clean = torch.from_numpy(_fill(lay, 7)).cuda().nan_to_num_(nan=0.0)  # finite everywhere: the guard says ok
    bad1_host = _fill(lay, 7, [(begins[names.index("odd")] + 17, float("nan"))])
    bad2_host = _fill(lay, 7, [(begins[names.index("many")] + 5000, float("nan"))])
    bad1, bad2 = torch.from_numpy(bad1_host).cuda(), torch.from_numpy(bad2_host).cuda()
    call = _Call(lay, fill=0x5C)
    call.rec[0:4].zero_()  # armed; everything else is the byte pattern
    before = call.raw()
    guard, finalize = _guard_for(clean)
    assert finalize(clean) == (0, 0)
    assert call.run(clean, ML.STATS_ON_SKIP, guard) == 0
    assert call.raw() == before, "a clean step must leave the record byte for byte"  # ok = 1
    assert finalize(clean) == (0, 0)  # applied_steps = 2
    assert finalize(bad1) == (0, 0)   # gap NaNs and the planted one: ok = 0, skipped_steps = 1
    assert call.run(bad1, ML.STATS_ON_SKIP, guard) == 0
    first = call.raw()
    hdr = ML.MmtStatsHeader.from_buffer_copy(first[:32])
    assert (hdr.valid, hdr.nseg, hdr.applied_steps, hdr.skipped_steps) == (1, call.nseg, 2, 1)
    rep = call.report()
    _check(call, bad1_host, rep)
    assert rep.nonfinite() == [("odd", 1, 0, 17)]
    # a second faulty step, elsewhere: the first snapshot stays
    assert finalize(bad2) == (0, 0)
    assert call.run(bad2, ML.STATS_ON_SKIP, guard) == 0
    assert call.raw() == first
    # a clean step does not touch it either
    assert finalize(clean) == (0, 0)
    assert call.run(clean, ML.STATS_ON_SKIP, guard) == 0
    assert call.raw() == first
    # re-armed: the next faulty step is taken
    call.rec[0:4].zero_()
    assert finalize(bad2) == (0, 0)
    assert call.run(bad2, ML.STATS_ON_SKIP, guard) == 0
    rep2 = call.report()
    _check(call, bad2_host, rep2)
    assert rep2.nonfinite() == [("many", 1, 0, 5000)]
    assert (rep2.applied_steps, rep2.skipped_steps) == (3, 3)
    assert call.bands_intact()


def test_always_mode_copies_the_guard_counters():
    lay = _layout_b()
    x = torch.from_numpy(_fill(lay, 8)).cuda().nan_to_num_(nan=0.0)
    guard, finalize = _guard_for(x)
    for _ in range(3):
        assert finalize(x) == (0, 0)
    call = _Call(lay)
    assert call.run(x, ML.STATS_ALWAYS, guard) == 0
    rep = call.report()
    assert (rep.applied_steps, rep.skipped_steps) == (3, 0)


# ------------------------------------------------------------------------------------------------ arguments
def test_invalid_arguments():
    lay = _layout_a()
    call = _Call(lay)
    x = torch.from_numpy(_fill(lay, 9)).cuda()
    guard = torch.zeros(ML.lib().mmt_guard_state_bytes(), dtype=torch.uint8, device="cuda")
    good = dict(stream=_stream(), x=ML.ptr(x), n=x.numel(), seg=ML.ptr(call.table), nseg=call.nseg,
                mode=ML.STATS_ALWAYS, guard=None, scratch=ML.ptr(call.scratch), record=ML.ptr(call.rec))
    off = lambda t, k: ML.ptr(t.view(torch.uint8)[k:])  # noqa: E731
    before = call.raw()
    for bad in (dict(x=None), dict(seg=None), dict(scratch=None), dict(record=None), dict(nseg=-1), dict(n=-1),
                dict(x=off(x, 4)), dict(scratch=off(call.scratch, 8)), dict(record=off(call.rec, 8)),
                dict(mode=ML.STATS_ON_SKIP), dict(mode=ML.STATS_ON_SKIP, guard=off(guard, 8)), dict(mode=7)):
        assert ML.lib().mmt_tensor_stats(*{**good, **bad}.values()) == -1, bad  # MMT_ERR_INVALID
    assert call.raw() == before  # nothing was launched
    assert ML.lib().mmt_tensor_stats(*{**good, "x": None, "n": 0}.values()) == 0  # a null x is fine when n == 0
    rep = call.report()
    assert not rep.sqsum.any() and (rep.first_bad == -1).all()


# ------------------------------------------------------------------------------------------------ no host sync
class _FlatModel:
    """What TensorStats needs of a model: the flat parameter, its segment table and the stage ranges."""

    def __init__(self, layout):
        names, begins, ends, n = layout
        self.flat_params = torch.nn.Parameter(torch.from_numpy(_values(n, 10) * 0.02).cuda())
        bounds, named = mmt_stats.build_segments(names, begins, ends)
        self._seg = {"names": names, "begins": begins, "ends": ends, "bounds": bounds, "named": named,
                     "device": torch.tensor(bounds, dtype=torch.int64).cuda()}

    def tensor_segments(self):
        return self._seg

    def backward_stage_ranges(self):
        n = self.flat_params.numel()
        return [(n // 2, n), (0, n // 2)]


@pytest.mark.parametrize("mode", ["skipped", "every"])
def test_record_and_guarded_step_do_not_sync(mode):
    lay = _layout_a()
    m = _FlatModel(lay)
    stats = mmt_stats.TensorStats(m, mode)
    other = torch.nn.Parameter(torch.zeros(1027, device="cuda"))
    opt = mmt_optim.AdamW([m.flat_params, other], lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True, stats=stats)
    g_host = _fill(lay, 12)
    np.nan_to_num(g_host, copy=False, nan=0.0)
    m.flat_params.grad = torch.from_numpy(g_host * 1e-3).cuda()
    other.grad = torch.ones(1027, device="cuda")
    poisoned = m.flat_params.grad.clone()
    poisoned[lay[1][lay[0].index("two")] + 4000] = float("nan")
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()  # the first step: allocates the guard state and the moments
        opt.step()
        m.flat_params.grad.copy_(poisoned)
        opt.step()  # skipped
        if mode == "every":
            stats.record(m.flat_params.grad)
        with pytest.raises(RuntimeError):  # the mode is live in this build: a real sync raises
            stats.read()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert opt.counters()[:2] == (2, 1)
    rep = stats.read()
    assert rep.nonfinite() == [("two", 1, 0, 4000)]
    assert (rep.applied_steps, rep.skipped_steps) == ((2, 1) if mode == "skipped" else (0, 0))
    assert rep.first_poisoned_stage == 1  # the tensor begins in the lower half, which the second stage finalises
    assert stats.read() is None  # re-armed by the read above


def test_plain_optimizer_records_every_step():
    lay = _layout_b()
    m = _FlatModel(lay)
    stats = mmt_stats.TensorStats(m, "every")
    opt = mmt_optim.AdamW([m.flat_params], lr=1e-3, stats=stats)
    g_host = _fill(lay, 13)
    m.flat_params.grad = torch.from_numpy(g_host).cuda()
    opt.step()
    rep = stats.read()
    ref = _reference(g_host, lay[1], lay[2])[0]
    assert abs(float(rep.sqsum[0]) - ref[0]) <= (lay[2][0] - lay[1][0]) * U * ref[0]
    assert (rep.applied_steps, rep.skipped_steps) == (0, 0)  # no guard: no device step count
