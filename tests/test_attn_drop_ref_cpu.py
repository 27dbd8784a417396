"""The CPU reference of the attention dropout tests (tests/attn_drop_ref.py) against the oracle's masks, against
itself (pack / unpack), and the discrimination of the read-outs: one flipped keep bit must move the output element
that reads it by at least 4x that element's tolerance and leave every other element within its own."""
import numpy as np
import pytest

import attn_drop_ref as R
import mmt_oracle as O


@pytest.mark.parametrize("seed,p,l,i,site", [(1234, 0.1, 0, 0, O.SITE_SA_PROB), (0xDEADBEEF12345678, 0.5, 2, 3, O.SITE_CA_PROB)])
def test_keep_matrix_is_the_oracle_mask(seed, p, l, i, site):
    B, H, T = 2, 3, 37
    hd = O.HashDropout(seed, p)
    assert hd.thr == R.thr_of(p) and hd.scale == R.scale_of(p)
    for j in range(3):
        K = R.keep_matrix(hd.key(l, i, site), j, B, H, T, hd.thr)
        assert K.shape == (B, H, T, T) and K.dtype == bool
        for h in range(H):
            ref = hd.probs(l, i, site, j, h, H, B, T).numpy() != 0
            assert np.array_equal(K[:, h], ref), (j, h)
        # the padded form agrees inside T and hashes row bh*T + t past it (the next head slot's rows)
        Kp = R.keep_matrix(hd.key(l, i, site), j, B, H, T, hd.thr, padded=True)
        assert Kp.shape == (B, H, 64, 64) and np.array_equal(Kp[:, :, :T, :T], K)
        assert np.array_equal(Kp[0, 0, T:2 * T if 2 * T < 64 else 64, :T], K[0, 1, : 64 - T])
    assert 0.05 < 1.0 - K.mean() < 0.95  # some kept, some dropped


def test_keep_matrix_law_scalar():
    """One element by the law as AttnProblem states it, in python integers."""
    key, j, B, H, T, thr = 0x9ABCDEF1, 2, 2, 3, 45, R.thr_of(0.5)
    K = R.keep_matrix(key, j, B, H, T, thr)
    for (b, h, t, s) in [(0, 0, 0, 0), (1, 2, 44, 43), (1, 0, 17, 6), (0, 1, 30, 31)]:
        dk = int(O.mask_hash(key, j, O.STREAM_SALT))
        rh = int(O.mask_hash(dk, (b * H + h) * T + t, O.PROB_ROW_SALT))
        hk = int(O.prob_hash(rh, s >> 1))
        assert bool(K[b, h, t, s]) == (((hk >> ((s & 1) * 16)) & 0xFFFF) >= thr)


@pytest.mark.parametrize("T", [1, 33, 96])
def test_pack_unpack_round_trip(T):
    B, H = 2, 3
    nt = (T + 31) // 32
    K = R.keep_matrix(77 + T, 1, B, H, T, R.thr_of(0.5), padded=True)
    rec = R.pack_records(K, B, H, T)
    assert rec.dtype == np.uint32 and rec.shape == (2 * 32 * R.ntiles(B, H, T),)
    km, lw = R.unpack_records(rec, B, H, T, padded=True)
    tile_ok = np.kron(np.tril(np.ones((nt, nt), dtype=bool)), np.ones((32, 32), dtype=bool))
    for got in (km, lw):
        assert np.array_equal(got[:, :, tile_ok], K[:, :, tile_ok])
        assert not got[:, :, ~tile_ok].any()
    km_c, lw_c = R.unpack_records(rec, B, H, T)
    assert np.array_equal(km_c, km[:, :, :T, :T]) and np.array_equal(lw_c, lw[:, :, :T, :T])


def test_pack_records_layout_by_hand():
    """One set bit lands where AttnProblem::dmask says, in both records."""
    B, H, T = 1, 2, 70  # nt = 3, ntri = 6
    for (bh, t, s) in [(0, 0, 0), (1, 69, 37), (1, 40, 5), (0, 63, 63), (1, 95, 64)]:
        K = np.zeros((B, H, 96, 96), dtype=bool)
        K[0, bh, t, s] = True
        rec = R.pack_records(K, B, H, T)
        qt, kt, r, kk = t // 32, s // 32, t % 32, s % 32
        tile = bh * 6 + qt * (qt + 1) // 2 + kt
        u = (kk >> 2) & 1
        e = (kk & 3) + 4 * (kk >> 3)
        assert kk == (e & 3) + 8 * (e >> 2) + 4 * u
        want = np.zeros_like(rec)
        want[tile * 32 + 2 * e + u] = 1 << r
        lane = r + 32 * u
        bit = (e >> 1) + 8 * (e & 1)
        want[(12 + tile) * 32 + (lane >> 1)] = 1 << (bit + 16 * (lane & 1))
        assert np.array_equal(rec, want), (bh, t, s)


def test_selector_and_windows():
    T, hs = 37, 16
    assert R.nwindows(T, hs) == 3
    E = np.arange(T * T, dtype=np.float64).reshape(T, T)
    for w in range(3):
        s = R.sel_window(T, hs, w)
        assert s.shape == (T, hs) and s.sum() == min(hs, T - w * hs)
        assert np.array_equal(R.window_cols(E, w, hs), E @ s)
        assert np.array_equal(R.window_rows(E, w, hs), E.T @ s)


def _flip_check(full, T, exempt_row0, same_row_free):
    """full(K) -> (E, tol) [T, T]. Every single-bit flip (s <= t): the element (t, s) moves by >= 4x its
    tolerance (the larger of before / after); no other element moves by more than its own (same_row_free: the
    other elements of row t may, the closed form says so). Returns the smallest ratio."""
    rng = np.random.default_rng(0)
    K = np.tril(rng.random((T, T)) < 0.7)
    worst = np.inf
    E0, tol0 = full(K)
    for t in range(T):
        for s in range(t + 1):
            K2 = K.copy()
            K2[t, s] = not K2[t, s]
            E1, tol1 = full(K2)
            d = np.abs(E1 - E0)
            tol = np.maximum(tol0, tol1)
            if not (exempt_row0 and t == 0):
                assert d[t, s] >= 4.0 * tol[t, s] and d[t, s] > 0.0, (t, s, d[t, s], tol[t, s])
                if tol[t, s] > 0:
                    worst = min(worst, d[t, s] / tol[t, s])
            d[t, s] = 0.0
            if same_row_free:
                d[t, :] = 0.0
            assert (d <= tol).all(), (t, s)
    return worst


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("hs", [16, 32, 64])
def test_single_bit_flip_moves_its_element_forward_and_dv(hs, p):
    T = 96
    c = R.scale_of(p)
    for tolf in (R.tol_fwd, R.tol_dv):
        def full(K):
            E = R.readout_keep(K, c)
            return E, tolf(E)
        worst = _flip_check(full, T, False, False)
        assert worst >= 64.0  # c/(t+1) against 2^-7 or 2^-6 of it


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("hs", [16, 32, 64])
def test_single_bit_flip_moves_its_element_dq(hs, p):
    T = 96
    c = R.scale_of(p)
    rng = np.random.default_rng(hs)
    v, do = R.grid_values((T, hs), rng), R.grid_values((T, hs), rng)
    worst = _flip_check(lambda K: R.readout_dq([K], c, [v], do, hs ** -0.5), T, True, True)
    print(f"dq read-out hs {hs} p {p}: smallest flip / tolerance ratio {worst:.1f}")
    assert worst >= 4.0


def test_readouts_batched_equal_per_head():
    """The closed forms broadcast over leading (b, h) dims as the GPU tests use them."""
    rng = np.random.default_rng(5)
    B, H, T, hs = 2, 3, 37, 16
    K = [R.keep_matrix(9, j, B, H, T, R.thr_of(0.5)) for j in range(2)]
    v = [R.grid_values((B, H, T, hs), rng) for _ in range(2)]
    do = R.grid_values((B, H, T, hs), rng)
    E, tol = R.readout_dq(K, 2.0, v, do, 0.25)
    e01, t01 = R.readout_dq([k[1, 2] for k in K], 2.0, [x[1, 2] for x in v], do[1, 2], 0.25)
    assert np.array_equal(E[1, 2], e01) and np.array_equal(tol[1, 2], t01)
    assert np.array_equal(R.readout_keep(K[0], 2.0)[0, 1], R.readout_keep(K[0][0, 1], 2.0))
    # p = 0.5 has rows with every key dropped: their D is 0 and so is the row
    dead = ~np.tril(K[0]).any(-1)
    assert dead.any()
    E1, _ = R.readout_dq(K[:1], 2.0, v[:1], do, 0.25)
    assert (E1[dead] == 0).all()
