"""Attention-probability dropout at kernel level (include/mmt.h: mmt_op_attention_mask, _fwd_drop, _bwd_drop).

1. The keep-bit records of attn_mask_kernel, both packings, bit for bit against tests/attn_drop_ref.py
   (pack_records(keep_matrix(...))) with torch.equal, 64-dword guard bands on both sides of every buffer, for
   every tiles-per-wave setting of mmt_attn_set_mask_g. The kernel's 64-bit index branch (more than 0x7fffffff
   tiles in a launch) cannot be reached at a test's size (it needs 256 GB of records) and is not tried.

2. The bits as each attention kernel consumes them. With q = 0 every score is 0, P[t, s] = 1/(t+1) and lse =
   log2(t+1) whatever the mask, and a selector window (sel_w[s, d] = (s == w*hs + d), exact in bf16) as V, dO or K
   turns one keep bit into one output element with a closed-form value (attn_drop_ref: readout_keep,
   readout_dq). One wrong bit is a 100 % error of one element; the tolerances are a few bf16 roundings, derived
   in attn_drop_ref (tol_fwd 2^-7, tol_dv 2^-6, readout_dq), not measured. One launch per window reads every bit
   of the record the kernel decodes: the forward and the dQ pass the lane words, the dK/dV pass the key-major
   dwords. Every test prints its largest error / tolerance ratio (DESIGN.md section 6 has the table).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attn_drop_ref as R
import attn_plan as AP
import mmt_lib as ML

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 64  # dwords on either side of a record buffer
PAD = 8  # sentinel columns behind every output row
PAD_VAL = -777.0  # (-776 in bf16)
MAX_STREAMS = 8
SENT32 = int(np.array([R.SENTINEL], dtype=np.uint32).view(np.int32)[0])


def _s():
    return ML.stream_ptr()


@functools.lru_cache(maxsize=64)
def _keep(key, j, B, H, T, thr, padded=False):
    """Host keep matrix, cached per (key, shape): shared by the tests of one path, never written."""
    K = R.keep_matrix(key, j, B, H, T, thr, padded=padded)
    K.setflags(write=False)
    return K


@functools.lru_cache(maxsize=64)
def _records(key, j, B, H, T, thr):
    rec = R.pack_records(_keep(key, j, B, H, T, thr, True), B, H, T)
    return torch.from_numpy(rec.view(np.int32).copy())


def _mask_buffers(B, H, T, nstreams):
    """Per problem, per stream: int32 [GUARD + dwords + GUARD] full of the sentinel."""
    nd = ML.lib().mmt_op_attention_mask_dwords(B, H, T)
    assert nd == 64 * R.ntiles(B, H, T)
    return nd, [[torch.full((nd + 2 * GUARD,), SENT32, dtype=torch.int32, device=DEV) for _ in range(ns)]
                for ns in nstreams]


def _launch_mask(B, T, H, nstreams, keys, thrs, bufs):
    cnt = len(nstreams)
    ptrs = (ctypes.c_void_p * (cnt * MAX_STREAMS))()
    for g in range(cnt):
        for j in range(nstreams[g]):
            ptrs[g * MAX_STREAMS + j] = bufs[g][j].data_ptr() + 4 * GUARD
    rc = ML.lib().mmt_op_attention_mask(_s(), cnt, B, T, H, (ctypes.c_int32 * cnt)(*nstreams),
                                        (ctypes.c_uint32 * cnt)(*keys), (ctypes.c_uint32 * cnt)(*thrs), ptrs)
    assert rc == 0, rc
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------- 1. the records
def _check_records(B, H, T, nstreams, keys, thrs, gs):
    L = ML.lib()
    old = L.mmt_attn_set_mask_g(0)
    try:
        for g in gs:
            L.mmt_attn_set_mask_g(g)
            nd, bufs = _mask_buffers(B, H, T, nstreams)
            _launch_mask(B, T, H, nstreams, keys, thrs, bufs)
            for pi, ns in enumerate(nstreams):
                for j in range(ns):
                    got = bufs[pi][j].cpu()
                    assert (got[:GUARD] == SENT32).all() and (got[GUARD + nd:] == SENT32).all(), (g, pi, j)
                    if thrs[pi] == 0:  # no dropout: nothing is written
                        assert (got == SENT32).all(), (g, pi, j)
                        continue
                    want = _records(keys[pi], j, B, H, T, thrs[pi])
                    pay = got[GUARD:GUARD + nd]
                    if not torch.equal(pay, want):
                        bad = (pay != want).nonzero().flatten()
                        nt32 = 32 * R.ntiles(B, H, T)
                        d = int(bad[0])
                        raise AssertionError(f"G {g} problem {pi} stream {j}: {bad.numel()} dwords differ, first: "
                                             f"{'key-major' if d < nt32 else 'lane-word'} record, tile {d % nt32 // 32}, "
                                             f"dword {d % 32}, bits {int(pay[d]) ^ int(want[d]):#x}")
    finally:
        L.mmt_attn_set_mask_g(old)


ALL_G = [1, 2, 4, 8, 16]
THRS = [R.thr_of(0.1), R.thr_of(0.5)]


@pytest.mark.parametrize("thr", THRS)
def test_records_single_tile(thr):
    """B*H = 1, T = 1: one tile; the wave has ng = 1 < G and three of the block's four waves have nothing."""
    _check_records(1, 1, 1, [1], [0x1234567], [thr], ALL_G)


@pytest.mark.parametrize("thr", THRS + [1, 65535])
def test_records_walk_crosses_every_boundary(thr):
    """B = 1, H = 3, T = 33, two streams: 3 tiles per (b, h), 9 per stream, 18 in all; for every G > 1 some wave
    crosses a query tile, a (b, h) and the stream boundary mid-walk. Also the extreme thresholds."""
    _check_records(1, 3, 33, [2], [0xC0FFEE11], [thr], ALL_G)


@pytest.mark.parametrize("thr", THRS)
def test_records_ragged_asymmetric(thr):
    """B = 2, H = 3, T = 100, three streams: bh = b*H + h with B != H, ragged last tile."""
    _check_records(2, 3, 100, [3], [0x9E3779B9], [thr], ALL_G)


@pytest.mark.parametrize("thr", THRS)
def test_records_batch_of_problems(thr):
    """count = 3 with 1, 3 and 2 streams, the middle one without dropout: the grid is sized by the widest problem
    and the narrower ones stop at their own total; the drop_thr = 0 problem's buffers keep the sentinel."""
    _check_records(2, 3, 33, [1, 3, 2], [0x11111111, 0x22222222, 0x33333333], [thr, 0, thr], ALL_G)


@pytest.mark.parametrize("thr", THRS)
def test_records_t1024(thr):
    """B*H = 2, T = 1024: nt = 32; the knob at 0 takes G = 16 by default at this T."""
    _check_records(2, 1, 1024, [1], [0xABCDEF01], [thr], ALL_G + [0])


@pytest.mark.parametrize("thr", THRS)
def test_records_t4096(thr):
    """B*H = 1, T = 4096: ntri = 8256, the float sqrtf triangle root at its largest; 2 MB of records."""
    _check_records(1, 1, 4096, [1], [0x0BADF00D], [thr], [8, 16])


def test_mask_op_refuses_bad_arguments():
    L = ML.lib()
    nd, bufs = _mask_buffers(1, 1, 1, [1])
    ptrs = (ctypes.c_void_p * MAX_STREAMS)()
    ptrs[0] = bufs[0][0].data_ptr() + 4 * GUARD
    one, key, thr = (ctypes.c_int32 * 9)(*[1] * 9), (ctypes.c_uint32 * 9)(*[5] * 9), (ctypes.c_uint32 * 9)(*[7] * 9)
    many = (ctypes.c_void_p * (9 * MAX_STREAMS))()
    assert L.mmt_op_attention_mask(_s(), 0, 1, 1, 1, one, key, thr, ptrs) == -1
    assert L.mmt_op_attention_mask(_s(), 9, 1, 1, 1, one, key, thr, many) == -1
    assert L.mmt_op_attention_mask(_s(), 1, 1, 1, 1, None, key, thr, ptrs) == -1
    assert L.mmt_op_attention_mask(_s(), 1, 1, 1, 1, one, None, thr, ptrs) == -1
    assert L.mmt_op_attention_mask(_s(), 1, 1, 1, 1, one, key, None, ptrs) == -1
    assert L.mmt_op_attention_mask(_s(), 1, 1, 1, 1, one, key, thr, None) == -1
    assert L.mmt_op_attention_mask(_s(), 1, 1, 1, 1, (ctypes.c_int32 * 1)(9), key, thr, ptrs) == -1
    assert L.mmt_op_attention_mask(_s(), 1, 1, 1, 1, one, key, thr, (ctypes.c_void_p * MAX_STREAMS)()) == -1
    torch.cuda.synchronize()
    assert (bufs[0][0] == SENT32).all()  # nothing launched


# --------------------------------------------------------------------------------- 2. the read-outs
class _Problem:
    """Buffers of one attention problem in the cross-attention layout (q [R, C]; per stream K and V rows
    [R, C], head h at column h*hs), outputs with PAD sentinel columns per row, NaN where a kernel must write."""

    def __init__(self, B, T, H, hs, ns, p, key, scratch):
        self.B, self.T, self.H, self.hs, self.ns = B, T, H, hs, ns
        self.R, self.C = B * T, H * hs
        self.key, self.thr, self.c = key, R.thr_of(p), R.scale_of(p)
        self.scale = hs ** -0.5
        R_, C = self.R, self.C
        self.q = torch.zeros(R_, C, dtype=torch.bfloat16, device=DEV)
        self.k = [torch.zeros(R_, C, dtype=torch.bfloat16, device=DEV) for _ in range(ns)]
        self.v = [torch.zeros(R_, C, dtype=torch.bfloat16, device=DEV) for _ in range(ns)]
        self.do = torch.zeros(R_, C, dtype=torch.bfloat16, device=DEV)
        self.o = self._out()
        self.oj = [self._out() for _ in range(ns)]
        self.lse = [torch.full((B * H * T,), NAN, device=DEV) for _ in range(ns)]
        self.dvec = [torch.zeros(B * H * T, device=DEV) for _ in range(ns)]
        self.dq = self._out()
        self.dk = [self._out() for _ in range(ns)]
        self.dv = [self._out() for _ in range(ns)]
        self.dq32 = torch.full((R_, C + 4), NAN, device=DEV) if scratch else None
        # the keep bits, from the library on the same key (section 1 has shown them right)
        self.nd, mb = _mask_buffers(B, H, T, [ns])
        self.mbuf = mb[0]
        _launch_mask(B, T, H, [ns], [key], [self.thr], mb)
        self.mptr = (ctypes.c_void_p * ns)(*[b.data_ptr() + 4 * GUARD for b in self.mbuf])
        self.keep = [_keep(key, j, B, H, T, self.thr) for j in range(ns)]

    def _out(self):
        t = torch.full((self.R, self.C + PAD), NAN, dtype=torch.bfloat16, device=DEV)
        t[:, self.C:] = PAD_VAL
        return t

    def _poison(self, ts):
        for t in ts:
            t[:, : self.C] = NAN

    def rows(self, a):
        """[B, H, T, hs] (or [T, hs], the same for every b, h) numpy -> bf16 [R, C] device rows."""
        a = np.asarray(a, dtype=np.float32)
        if a.ndim == 2:
            a = np.broadcast_to(a, (self.B, self.H) + a.shape)
        t = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1, 3))).reshape(self.R, self.C)
        out = t.to(torch.bfloat16)
        assert torch.equal(out.float(), t)  # the inputs are exact in bf16
        return out.to(DEV)

    def heads(self, t):
        """Output rows [R, C + PAD] -> fp64 numpy [B, H, T, hs]; the pad columns must hold the sentinel."""
        assert (t[:, self.C:].float() == torch.tensor(PAD_VAL).bfloat16().float()).all(), "pad columns written"
        a = t[:, : self.C].float().cpu().numpy().astype(np.float64)
        return a.reshape(self.B, self.T, self.H, self.hs).transpose(0, 2, 1, 3)

    def _ptrs(self, ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def forward(self):
        self._poison([self.o] + self.oj)
        for l in self.lse:
            l.fill_(NAN)
        rc = ML.lib().mmt_op_attention_fwd_drop(
            _s(), self.B, self.T, self.H, self.hs, self.ns, ML.ptr(self.q), self.C, self._ptrs(self.k),
            self._ptrs(self.v), self.C, self.hs, ML.ptr(self.o), self.C + PAD, self._ptrs(self.oj), self._ptrs(self.lse),
            self.key, self.thr, self.c, self.mptr)
        assert rc == 0, rc
        torch.cuda.synchronize()

    def backward(self):
        self._poison([self.dq] + self.dk + self.dv)
        if self.dq32 is not None:
            self.dq32.fill_(NAN)
        rc = ML.lib().mmt_op_attention_bwd_drop(
            _s(), self.B, self.T, self.H, self.hs, self.ns, ML.ptr(self.q), self.C, self._ptrs(self.k),
            self._ptrs(self.v), self.C, self.hs, ML.ptr(self.o), self.C + PAD, self._ptrs(self.oj), self._ptrs(self.lse),
            ML.ptr(self.do), self.C, self._ptrs(self.dvec), ML.ptr(self.dq), self.C + PAD, self._ptrs(self.dk),
            self._ptrs(self.dv), self.C + PAD, self.hs, ML.ptr(self.dq32), (self.C + 4) if self.dq32 is not None else 0,
            self.key, self.thr, self.c, self.mptr)
        assert rc == 0, rc
        torch.cuda.synchronize()

    def check_mask_untouched(self):
        for j, b in enumerate(self.mbuf):
            got = b.cpu()
            assert (got[:GUARD] == SENT32).all() and (got[GUARD + self.nd:] == SENT32).all()
            assert torch.equal(got[GUARD:GUARD + self.nd], _records(self.key, j, self.B, self.H, self.T, self.thr))


def _ratio(got, want, tol, what):
    """Largest |got - want| / tol over the elements with tol > 0; where tol == 0 (an expected 0) got must be
    exactly +-0. NaN anywhere fails."""
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} elements not written (NaN)"
    zero = tol == 0
    assert (want[zero] == 0).all()
    if (got[zero] != 0).any():
        i = np.argwhere(zero & (got != 0))[0]
        raise AssertionError(f"{what}: element {tuple(i)} is {got[tuple(i)]}, expected exactly 0")
    r = np.abs(got - want)[~zero] / tol[~zero]
    return float(r.max()) if r.size else 0.0


def _fail_where(got, want, tol, what):
    bad = np.argwhere(np.abs(got - want) > tol)
    i = tuple(bad[0])
    return (f"{what}: {len(bad)} elements out of tolerance, first (b, h, row, col) = {i}: got {got[i]}, "
            f"expected {want[i]}, tolerance {tol[i]}")


def _lse_check(P):
    T = P.T
    want = np.log2(np.arange(1, T + 1, dtype=np.float64))
    tol = 4 * np.spacing(np.maximum(want, 1.0).astype(np.float32)).astype(np.float64)
    for j in range(P.ns):
        got = P.lse[j].cpu().numpy().astype(np.float64).reshape(P.B, P.H, T)
        assert np.isfinite(got).all()
        assert (np.abs(got - want) <= tol).all(), (j, np.abs(got - want).max())


def _readout_fwd(P):
    E = [R.readout_keep(K, P.c) for K in P.keep]
    worst = 0.0
    for w in range(R.nwindows(P.T, P.hs)):
        sel = P.rows(R.sel_window(P.T, P.hs, w))
        for v in P.v:
            v.copy_(sel)
        P.forward()
        _lse_check(P)
        wj = [R.window_cols(e, w, P.hs) for e in E]
        if P.ns > 1:
            for j in range(P.ns):
                got = P.heads(P.oj[j])
                tol = R.tol_fwd(wj[j])
                r = _ratio(got, wj[j], tol, f"oj[{j}] window {w}")
                assert r <= 1.0, _fail_where(got, wj[j], tol, f"oj[{j}] window {w}")
                worst = max(worst, r)
        got = P.heads(P.o)
        want, tol = sum(wj), R.tol_fwd(sum(np.abs(x) for x in wj))
        r = _ratio(got, want, tol, f"o window {w}")
        assert r <= 1.0, _fail_where(got, want, tol, f"o window {w}")
        worst = max(worst, r)
    return worst


def _grid_inputs(P, seed):
    rng = np.random.default_rng(seed)
    shp = (P.B, P.H, P.T, P.hs)
    v = [R.grid_values(shp, rng) for _ in range(P.ns)]
    do = R.grid_values(shp, rng)
    k = [R.grid_values(shp, rng) for _ in range(P.ns)]
    return k, v, do


def _readout_dv(P):
    k, v, _ = _grid_inputs(P, 11)
    for j in range(P.ns):
        P.k[j].copy_(P.rows(k[j]))
        P.v[j].copy_(P.rows(v[j]))
    P.forward()
    _lse_check(P)
    E = [R.readout_keep(K, P.c) for K in P.keep]
    worst = 0.0
    for w in range(R.nwindows(P.T, P.hs)):
        P.do.copy_(P.rows(R.sel_window(P.T, P.hs, w)))
        P.backward()
        for j in range(P.ns):
            got = P.heads(P.dv[j])
            want = R.window_rows(E[j], w, P.hs)
            tol = R.tol_dv(want)
            r = _ratio(got, want, tol, f"dv[{j}] window {w}")
            assert r <= 1.0, _fail_where(got, want, tol, f"dv[{j}] window {w}")
            worst = max(worst, r)
            # q = 0: dK = scale dS^T Q is exactly 0, and written
            dk = P.heads(P.dk[j])
            assert np.isfinite(dk).all() and not dk.any(), f"dk[{j}] window {w}"
        assert np.isfinite(P.heads(P.dq)).all(), f"dq window {w} not written"
    return worst


def _readout_dq(P):
    _, v, do = _grid_inputs(P, 12)
    for j in range(P.ns):
        P.v[j].copy_(P.rows(v[j]))
    P.do.copy_(P.rows(do))
    P.forward()
    _lse_check(P)
    E, tol = R.readout_dq(P.keep, P.c, v, do, P.scale)
    worst = 0.0
    for w in range(R.nwindows(P.T, P.hs)):
        sel = P.rows(R.sel_window(P.T, P.hs, w))
        for kk in P.k:
            kk.copy_(sel)
        P.backward()
        got = P.heads(P.dq)
        want, tw = R.window_cols(E, w, P.hs), R.window_cols(np.ascontiguousarray(tol), w, P.hs)
        r = _ratio(got, want, tw, f"dq window {w}")
        assert r <= 1.0, _fail_where(got, want, tw, f"dq window {w}")
        worst = max(worst, r)
        for j in range(P.ns):
            assert np.isfinite(P.heads(P.dk[j])).all() and np.isfinite(P.heads(P.dv[j])).all(), f"window {w}"
    return worst


# (path, mmt_attn_set_ring, hs, T, streams, fp32 dQ scratch): attn_plan.PATHS, with the kernels each path names
PATHS = AP.PATHS
READOUTS = {"fwd": _readout_fwd, "dv": _readout_dv, "dq": _readout_dq}


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("readout", ["fwd", "dv", "dq"])
@pytest.mark.parametrize("path,ring,hs,T,ns,scratch", PATHS, ids=[f"{a[0]}-hs{a[2]}-T{a[3]}-ns{a[4]}" for a in PATHS])
def test_readout(path, ring, hs, T, ns, scratch, readout, p):
    """Every keep bit of B = 2, H = 3 (bh = b*H + h is not symmetric) as the kernels of `path` consume it; p = 0.5
    has rows with every key dropped."""
    L = ML.lib()
    B, H = 2, 3
    old = L.mmt_attn_set_ring(ring)
    try:
        # the launches below take the kernels the row is named for (the plan: host arithmetic, no launch)
        fwd, bwd = AP.PATH_FAMILIES[path]
        assert AP.families(L, AP.readout_call(AP.FWD, T, hs, ns, scratch)) == (fwd,)
        assert AP.families(L, AP.readout_call(AP.BWD, T, hs, ns, scratch)) == bwd
        P = _Problem(B, T, H, hs, ns, p, 0x5EED0000 + 64 * hs + ns, scratch)
        if p == 0.5:
            assert (~np.tril(P.keep[0]).any(-1)).any()
        worst = READOUTS[readout](P)
        P.check_mask_untouched()
    finally:
        L.mmt_attn_set_ring(old)
    print(f"readout {readout:3s} {path} ring {ring} hs {hs} T {T} streams {ns} p {p}: max error / tolerance {worst:.3f}")
    assert worst <= 1.0
