"""tests/exact_ref.py on the CPU: the rounding helper, the order-independence condition on every input set of
tests/test_gpu_exact_kernels.py at its largest shape, fp32 sums in random orders against the fp64 reference, and
the FFN / mlp2_bwd references against a plain torch fp32 composition of the existing tests' formulas."""
import numpy as np
import pytest
import torch

import exact_ref as E


def _bits(t):
    return t.view(torch.int16)


def test_rne_bf16_ties_and_non_ties():
    """Between 256 and 512 bf16 numbers are 2 apart: odd integers are ties and go to the even significand."""
    x = torch.tensor([257.0, 259.0, 258.0, 261.0, 256.5, 257.5, -257.0, -259.0, -258.0, 1.00390625, 1.01171875, 0.0, -0.0])
    want = torch.tensor([256.0, 260.0, 258.0, 260.0, 256.0, 258.0, -256.0, -260.0, -258.0, 1.0, 1.015625, 0.0, -0.0])
    got = E.rne_bf16(x)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got.float(), want)
    assert _bits(got)[-2].item() == 0 and _bits(got)[-1].item() == -32768  # +0 is 0x0000, -0 is 0x8000
    assert torch.equal(E.rne_bf16(x.double()).float(), want)  # fp64 input that is an fp32 number
    with pytest.raises(AssertionError):
        E.rne_bf16(torch.tensor([1.0 + 2.0 ** -40], dtype=torch.float64))  # would round twice


def test_generators_are_seeded_and_bf16_exact():
    a, b = E.ints((50, 60), -4, 4, 7), E.ints((50, 60), -4, 4, 7)
    assert torch.equal(a, b) and a.min() == -4 and a.max() == 4 and torch.equal(a, a.round())
    h = E.ints((50, 60), -2, 2, 8, step=0.25)
    assert torch.equal(h * 4, (h * 4).round()) and E.bf16_exact(h) and h.unique().numel() == 17
    c = E.choice((40, 40), [0.0, 0.5, -0.5, 1.0, -1.0], 9)
    assert set(c.unique().tolist()) == {0.0, 0.5, -0.5, 1.0, -1.0}
    z = E.signed_zeros(torch.zeros(1000), 3)
    neg = int(torch.signbit(z).sum())
    assert 300 < neg < 700 and bool((z == 0).all())
    with pytest.raises(AssertionError):
        E.ints((10, 10), 250, 300, 1)  # 257 is not a bf16 number


def test_assert_exact_accepts_and_refuses():
    a, b = torch.full((2, 1024), 4.0), torch.full((1024, 3), 3.0)
    assert E.assert_exact(a, b, extra=100.0) == 1024 * 12 + 100
    assert E.assert_exact(a, b, alpha=0.25, unit=0.25) == 1024 * 12
    with pytest.raises(AssertionError):
        E.assert_exact(torch.full((1, 1 << 16), 16.0), torch.full((1 << 16, 1), 16.0))  # 2^24: one unit too many
    with pytest.raises(AssertionError):
        E.assert_exact(torch.full((2, 8), 3.0), b[:8], alpha=0.5)  # 4.5 is no multiple of the unit 1
    with pytest.raises(AssertionError):
        E.assert_exact(a, b, extra=0.5)


def test_every_gpu_input_set_is_order_independent_at_its_largest_shape():
    """Each builder calls assert_exact on its own inputs (and f32_exact on its reference): building the largest
    case of every family runs those checks at the GPU file's largest K / R."""
    M, N, K = max(E.GEMM_SHAPES, key=lambda s: s[2])
    assert K == 1032
    c = E.gemm_fwd_case(M, N, K)
    for epi in ("store_f32", "bias_resid_f32", "store_bf16", "bias_relu_bf16"):
        E.gemm_fwd_want(c, epi)
    relu = E.gemm_fwd_want(c, "bias_relu_bf16")[1].float()
    assert bool((relu == 0).any()) and bool((relu > 256).any())  # both sides of 0, exactly 0, and rounded values
    pre = c["base"] + c["bias"].double()
    assert bool((pre == 0).any()) and bool((pre < 0).any()) and bool((pre > 0).any())
    ties = ((pre.abs() > 256) & (pre.abs() < 512) & (pre % 2 == 1)).float().mean().item()
    assert ties > 0.01, ties  # RNE ties: where truncation and round-half-up differ from RNE
    c = E.gemm_bwd_case(M, N, K)
    for epi in ("store_f32", "acc_f32", "store_bf16", "drelu_bf16", "dtanh_bf16"):
        for alpha in E.BWD_ALPHAS:
            E.gemm_bwd_want(c, epi, alpha)
    z = c["aux_relu"] == 0
    assert bool((z & torch.signbit(c["aux_relu"])).any()) and bool((z & ~torch.signbit(c["aux_relu"])).any())
    E.gemm_wgrad_case(M, N, K)
    E.gemm_wgrad_case(*max(E.WGRAD_SHAPES, key=lambda s: s[2]))
    E.colsum_case(1000, 450, 456)
    E.ordered_sum_case(40, 300)
    E.qkv2_case(*max(E.QKV2_SHAPES, key=lambda s: s[0] * s[2]))
    E.qkv2_case(1055, 3, 32)
    for alpha in (1.0, 0.5):
        E.mlp2_bwd_case(300, 512, alpha)
    E.ffn_case(200, 200)
    E.embedding_case(*max(E.EMB_SHAPES, key=lambda s: s[0] * s[1]))
    E.f8_case(*max(E.F8_SHAPES, key=lambda s: s[2]))


@pytest.mark.parametrize("kind", ["fwd", "bwd", "wgrad"])
def test_fp32_sums_in_random_orders_equal_the_reference(kind):
    """The fp32 sum of the products, accumulated serially in numpy float32 in three random orders of k, equals the
    fp64 reference bit for bit (a sample of 24 x 24 output elements at the largest K / R)."""
    if kind == "fwd":
        c = E.gemm_fwd_case(520, 328, 1032)
        a, b, ref = c["X"], c["W"].t(), c["base"]
    elif kind == "bwd":
        c = E.gemm_bwd_case(520, 328, 1032)
        a, b, ref = c["dY"], c["W"], c["base"]
    else:
        c = E.gemm_wgrad_case(384, 256, 4096)
        a, b, ref = c["dY"].t().contiguous(), c["X"], E.gemm64(c["dY"].t(), c["X"])
    rows, cols = torch.arange(0, a.shape[0], a.shape[0] // 24)[:24], torch.arange(0, b.shape[1], b.shape[1] // 24)[:24]
    want = ref[rows][:, cols].numpy()
    sums = E.sums_in_random_orders(a, b, rows, cols)
    assert len(sums) == 3
    for s in sums:
        assert s.dtype == np.float32
        assert np.array_equal(s.astype(np.float64), want)
        assert np.array_equal(s.view(np.int32), want.astype(np.float32).view(np.int32))


@pytest.mark.parametrize("M", [37, 200])
def test_ffn_reference_equals_torch_fp32_composition(M):
    """tests/test_gpu_ffn_fused.py's formulas in plain fp32 torch on the same inputs: exact there too."""
    c, w = E.ffn_case(M, 100 + M), E.ffn_weights()
    href = torch.relu(c["x"] @ w["w0"].t() + w["b0"])
    h = href.to(torch.bfloat16)
    out = c["resid"] + (h.float() @ w["w2"].t() + w["b2"])
    assert torch.equal(h, c["h"])
    assert torch.equal(out, c["out"])
    assert torch.equal(out.to(torch.bfloat16), c["out16"])
    assert bool((href > 256).any()) and not torch.equal(href, h.float())  # values above 256 occur and are rounded


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("M,C", [(130, 256), (300, 512)])
def test_mlp2_bwd_reference_equals_torch_fp32_composition(M, C, alpha):
    """tests/test_gpu_kernels.py test_mlp2_bwd_fused's formulas in plain fp32 torch: dref, its column sums, dx from
    the bf16 dh. The two db0 conventions differ on these inputs."""
    c = E.mlp2_bwd_case(M, C, alpha)
    dref = alpha * (c["dy"] @ c["w2"]) * (1 - c["h"] ** 2)
    dh = dref.to(torch.bfloat16)
    assert torch.equal(dh, c["dh"])
    assert torch.equal(c["pre"] + dref.sum(0), c["db0"])
    assert torch.equal((dh.float() @ c["w0"]).to(torch.bfloat16), c["dx"])
    assert not torch.equal(dref, dh.float())
    assert int((c["db0"].double() != c["db0_stored"]).sum()) > C // 8


def test_report_mismatch_names_count_places_and_pattern():
    want = torch.zeros(64, 16)
    got = want.clone()
    got[33, 8:16] = 1.0
    msg = E.report_mismatch(got, want, "case")
    assert "8 of 1024 elements differ" in msg and "(33, 8, 1.0, 0.0)" in msg
    assert "rows mod 32: [1]" in msg and "cols mod 8: [0, 1, 2, 3, 4, 5, 6, 7]" in msg
    assert "no differing element" in E.report_mismatch(want, want)
    assert "shape" in E.report_mismatch(want, want[:, :8])
