"""CPU reference of the attention-probability dropout: the keep law, the two packed keep-bit records of
AttnProblem::dmask (csrc/mmt_kernels.h), and the closed-form "read-outs" that turn one keep bit into one
output element of a forward or backward attention kernel. numpy / torch on the CPU only.

Keep law (csrc/mmt_common.h, AttnProblem): element (query t, key s) of stream j, head slot bh = b*H + h is kept
iff the 16-bit half (s & 1) of mmt_prob_hash(mmt_prob_row(mmt_hash(drop_key, j, STREAM_SALT), bh*T + t), s >> 1)
is >= thr. Built from the oracle's mask_hash / prob_hash (HashDropout.probs_raw).

Records, per stream: tile (bh, qt, kt <= qt) has index bh*ntri + qt(qt+1)/2 + kt (ntri = nt(nt+1)/2, nt =
ceil(T/32)); accumulator element e (0..15), half u, lane r of the tile stand for query qt*32 + r and key
kt*32 + (e&3) + 8(e>>2) + 4u. Key-major record (32 dwords per tile, tiles in index order): dword 2e + u, bit r.
Lane-word record (after all key-major records, 32 dwords per tile): 16 bits per lane r + 32u, element 2i at bit
i and element 2i + 1 at bit 8 + i; lane L's 16 bits are the half (L & 1) of dword L >> 1. Positions past T
inside the last tiles are hashed like any other (row bh*T + t, key s), so the records need the keep matrix padded
to 32*nt (keep_matrix(..., padded=True)).

Read-outs (q = 0, so every score is 0, P[t, s] = 1/(t+1) for s <= t and lse = log2(t+1), dropout or not; c =
drop_scale, K = keep matrix of one stream and head). Each is a [T, T] matrix E over (query t, key s) of which a
launch with the selector window sel_w (sel_w[s, d] = (s == w*hs + d), exact in bf16) shows hs columns or rows:
  forward  V = sel_w:                 o_j[t, d]  = E[t, w*hs + d],  E[t, s] = K[t, s] c / (t+1)
  dV       dO = sel_w over queries:   dV_j[s, d] = E[w*hs + d, s],  the same E
  dQ       K_j = sel_w:               dQ[t, d]   = sum_j E_j[t, w*hs + d],  E_j = scale * dS_j,
           dS_j = P (c K_j dP_j - D_j), dP_j = dO V_j^T, D_j[t] = sum_s P c K_j dP_j
Tolerances (derived, not measured; the derivations are in the functions' docstrings).
"""
import math

import numpy as np

import mmt_oracle as O

SENTINEL = 0xA5C3F00D


def thr_of(p):
    """The engine's 16-bit threshold of dropout probability p."""
    return int(min(65535.0, max(1.0, math.floor(p * 65536.0))))


def scale_of(p):
    """drop_scale: float32(1 / (1 - p))."""
    return float(np.float32(1.0 / (1.0 - p)))


def ntiles(B, H, T):
    nt = (T + 31) // 32
    return B * H * (nt * (nt + 1) // 2)


def keep_matrix(drop_key, j, B, H, T, thr, padded=False):
    """bool [B, H, T, T] (padded: [B, H, 32 nt, 32 nt], the positions the records also hold): the keep bits of
    stream j. Not restricted to s <= t."""
    n = (T + 31) // 32 * 32 if padded else T
    bh = (np.arange(B)[:, None] * H + np.arange(H)[None, :]).astype(np.int64)
    rows = bh[:, :, None] * T + np.arange(n, dtype=np.int64)[None, None, :]  # [B, H, n]
    return O.HashDropout.probs_raw(drop_key, j, rows[..., None], np.arange(n, dtype=np.int64)[None, None, None, :], thr)


# key offset inside a tile of accumulator element e, half u
_KK = np.array([[(e & 3) + 8 * (e >> 2) + 4 * u for u in range(2)] for e in range(16)])  # [16, 2]
# bit of element e in a lane word
_LW_BIT = np.array([(e >> 1) + 8 * (e & 1) for e in range(16)])


def _tiles(keep, B, H, T):
    """[B*H, ntri, 32 r, 32 key] lower-triangle tiles of a padded keep matrix, in record order."""
    nt = (T + 31) // 32
    n = nt * 32
    keep = np.asarray(keep, dtype=bool)
    assert keep.shape == (B, H, n, n), "pack_records needs the keep matrix padded to whole tiles (padded=True)"
    t = keep.reshape(B * H, nt, 32, nt, 32).transpose(0, 1, 3, 2, 4)  # [BH, qt, kt, r, kk]
    qt, kt = np.tril_indices(nt)  # row-major lower triangle: index qt(qt+1)/2 + kt
    return t[:, qt, kt]


def pack_records(keep, B, H, T):
    """uint32 [mask dwords] of one stream: the key-major records of every tile, then the lane-word records."""
    tl = _tiles(keep, B, H, T)
    bits = tl[..., _KK]  # [BH, ntri, r, e, u]
    ntl = bits.shape[0] * bits.shape[1]
    bits = bits.reshape(ntl, 32, 16, 2)
    km = (bits.transpose(0, 2, 3, 1).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1)  # [tile, e, u]
    km = km.astype(np.uint32).reshape(ntl, 32)  # dword 2e + u
    lw = (bits.transpose(0, 3, 1, 2).astype(np.uint32) << _LW_BIT.astype(np.uint32)).sum(-1)  # [tile, u, r]
    lw = lw.astype("<u2").reshape(ntl, 64).view("<u4").reshape(ntl, 32)  # lane r + 32u: half (L & 1) of dword L >> 1
    return np.concatenate([km.reshape(-1), lw.reshape(-1)]).astype(np.uint32)


def unpack_records(rec, B, H, T, padded=False):
    """The inverse: (key-major, lane-word) -> two bool [B, H, T, T] (padded: 32 nt) arrays, False outside the
    tiles kt <= qt."""
    nt = (T + 31) // 32
    n = nt * 32
    ntri = nt * (nt + 1) // 2
    ntl = B * H * ntri
    rec = np.asarray(rec, dtype=np.uint32)
    assert rec.shape == (2 * 32 * ntl,)
    km = rec[:32 * ntl].reshape(ntl, 16, 2)  # [tile, e, u]
    bits_km = ((km[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).transpose(0, 3, 1, 2)  # [tile, r, e, u]
    lw = rec[32 * ntl:].reshape(ntl, 32).astype("<u4").view("<u2").reshape(ntl, 2, 32)  # [tile, u, r]
    bits_lw = ((lw[..., None] >> _LW_BIT.astype(np.uint16)) & 1).astype(bool).transpose(0, 2, 3, 1)  # [tile, r, e, u]
    qt, kt = np.tril_indices(nt)
    outs = []
    for bits in (bits_km, bits_lw):
        tl = np.zeros((ntl, 32, 32), dtype=bool)
        tl[:, :, _KK] = bits
        full = np.zeros((B * H, nt, nt, 32, 32), dtype=bool)
        full[:, qt, kt] = tl.reshape(B * H, ntri, 32, 32)
        full = full.transpose(0, 1, 3, 2, 4).reshape(B, H, n, n)
        outs.append(full if padded else full[:, :, :T, :T].copy())
    return outs[0], outs[1]


# ------------------------------------------------------------------------------------------ read-outs
def nwindows(T, hs):
    return (T + hs - 1) // hs


def sel_window(T, hs, w):
    """float32 [T, hs]: sel_w[s, d] = (s == w*hs + d)."""
    s = np.zeros((T, hs), dtype=np.float32)
    d = np.arange(hs)
    ok = w * hs + d < T
    s[(w * hs + d)[ok], d[ok]] = 1.0
    return s


def grid_values(shape, rng):
    """Values on the positive grid {4..8}/8 (exact in bf16, products and short sums exact in fp32)."""
    return (rng.integers(4, 9, size=shape) / 8.0).astype(np.float32)


def window_cols(E, w, hs):
    """[..., T, hs]: columns w*hs .. w*hs + hs - 1 of E [..., T, T], zero past T."""
    T = E.shape[-1]
    out = np.zeros(E.shape[:-1] + (hs,), dtype=E.dtype)
    hi = min(T, (w + 1) * hs)
    out[..., : hi - w * hs] = E[..., w * hs:hi]
    return out


def window_rows(E, w, hs):
    """[..., T, hs]: out[s, d] = E[w*hs + d, s], zero past T (the dV read-out's view)."""
    return window_cols(np.swapaxes(E, -1, -2), w, hs)


def readout_keep(keep, c):
    """E[t, s] = K[t, s] c / (t+1) for s <= t, else 0 (fp64): the forward and the dV read-out.
    keep: bool [..., T, T]."""
    T = keep.shape[-1]
    t = np.arange(T, dtype=np.float64)
    E = np.tril(np.asarray(keep, dtype=np.float64)) * (np.float64(c) / (t + 1.0))[:, None]
    return E


def tol_fwd(E):
    """2^-7 |E| per stream (for the summed output: 2^-7 of the sum of magnitudes, tol_fwd of sum |E_j|): the
    kernel makes one fp32 c / l and one bf16 rounding, half an ulp = 2^-8 relative; the same again is slack for
    the order of p * inv. An expected 0 has tolerance 0: exactly +-0."""
    return np.abs(E) * 2.0 ** -7


def tol_dv(E):
    """2^-6 |E|: the recomputed P is rounded to bf16 for the MFMA (2^-8), and the sum times drop_scale is rounded
    to bf16 again (2^-8); twice that as slack. An expected 0 has tolerance 0."""
    return np.abs(E) * 2.0 ** -6


def readout_dq(keeps, c, vs, do, scale):
    """The dQ read-out of one (b, h)... or any leading dims: keeps list of bool [..., T, T], vs list of
    [..., T, hs], do [..., T, hs] (values as the kernel sees them). Returns (E, tol), fp64 [..., T, T]:
    E = scale * sum_j dS_j, tol[t, :] = 2^-6 scale c / (t+1) sum_j max_s dP_j[t, s] (covers the bf16 rounding of
    O_j inside D_j, of dS, and of dQ)."""
    T = do.shape[-2]
    t = np.arange(T, dtype=np.float64)
    P = np.tril(np.ones((T, T))) / (t + 1.0)[:, None]
    do = np.asarray(do, dtype=np.float64)
    E = 0.0
    tol = 0.0
    for K, v in zip(keeps, vs):
        dP = do @ np.swapaxes(np.asarray(v, dtype=np.float64), -1, -2)  # [..., T, T]
        Z = np.float64(c) * np.tril(np.asarray(K, dtype=np.float64))
        D = (P * Z * dP).sum(-1, keepdims=True)
        E = E + scale * P * (Z * dP - D)
        tol = tol + np.tril(dP).max(-1)
    tol = 2.0 ** -6 * scale * np.float64(c) / (t + 1.0) * tol
    return E, np.broadcast_to(tol[..., None], E.shape)
