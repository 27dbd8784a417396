"""The loss kernel of the training objective (mmt_op_cross_entropy_spec: the D pre-pass + the spec form of the
cross-entropy forward) against tests/loss_ref.py in fp64, at the sizes where the kernel's structure changes.

Shapes (R, T, V): V = 1, 2, 5, 13, 64 run the one-logit-per-lane instantiation, 65 just spills into the two-logit
one, 144 takes four, 300 eight, 900 sixteen and 1500 the three-pass form; R = 33 and 77 leave a ragged last block
of four rows, R = 4100 and 9000 (> 2048 = 512 blocks of 4 waves) make every wave walk several rows with a ragged
end. T = 11, 7, 41 and 125 do not divide 4, so a block's four rows straddle windows.

Bounds: those of test_cross_entropy (tests/test_gpu_kernels.py) for the plain kernel, which has the same fp32
sums and bf16 stores: rtol = atol = 1e-5 on the loss, rel-L2 < 1e-2 on the bf16 gradient. D is an fp64 sum of
exact products of fp32 numbers: 1e-12 relative against the reference's other summation order."""
import functools
import math

import pytest
import torch

import loss_ref
import mmt_lib as ML

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4  # sentinel rows behind row R

SHAPES = [(33, 11, 1), (77, 7, 2), (33, 11, 5), (77, 11, 13), (4100, 41, 64), (4100, 100, 65), (9000, 72, 144),
          (77, 7, 300), (4100, 41, 900), (9000, 125, 1500), (9000, 72, 5)]
VARIANTS = ["eps", "class", "position", "all"]


def r8(x):
    return max(8, (x + 7) // 8 * 8)


def rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-12)).item()  # as tests/test_gpu_kernels.py (V = 1: both are zero)


@functools.lru_cache(maxsize=4)
def _inputs(R, T, V):
    """logits, targets, class weights, position weights (a zero prefix of at least one position); never modified."""
    g = torch.Generator().manual_seed(R * 31 + V)
    x = (torch.randn(R, V, generator=g) * 2).to(DEV)
    t = torch.randint(0, V, (R,), generator=g).to(DEV)
    w = (torch.rand(V, generator=g) + 0.2).to(DEV)
    u = torch.rand(T, generator=g) + 0.5
    u[: max(1, T // 4)] = 0
    return x, t, w, u.to(DEV)


def _spec(variant, w, u):
    return {"eps": (0.1, None, None), "class": (0.0, w, None), "position": (0.0, None, u), "all": (0.1, w, u)}[variant]


def _run(x, t, T, eps, w, u, part=False, flag=False):
    R, V = x.shape
    ld = r8(V)
    dl = torch.full((R + GUARD, ld), 7.0, dtype=torch.bfloat16, device=DEV)
    loss = torch.zeros(1, device=DEV)
    denom = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    pbuf = torch.full((512,), float("nan"), device=DEV) if part else None
    fbuf = torch.zeros(2, dtype=torch.int32, device=DEV) if flag else None
    rc = ML.lib().mmt_op_cross_entropy_spec(ML.stream_ptr(), R, T, V, ML.ptr(x), ML.ptr(t), ML.ptr(dl), ld, ML.ptr(loss),
                                            eps, ML.ptr(w), ML.ptr(u), ML.ptr(denom), ML.ptr(pbuf), ML.ptr(fbuf))
    assert rc == 0
    torch.cuda.synchronize()
    return loss, dl, denom, fbuf


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("R,T,V", SHAPES)
def test_loss_and_gradient_against_the_reference(R, T, V, variant):
    x, t, w, u = _inputs(R, T, V)
    eps, cw, pw = _spec(variant, w, u)
    loss, dl, denom, _ = _run(x, t, T, eps, cw, pw)
    ref = loss_ref.objective(x, t, T, eps, cw, pw)
    grad = loss_ref.gradient(x, t, T, eps, cw, pw)
    D = float(loss_ref.denominator(t, T, cw, pw))
    got_d = float(denom[0])
    err_g = rel(dl[:R, :V].double() * (D / R ** 2), grad * (D / R))
    print(f"R={R} T={T} V={V} {variant}: loss {float(loss[0]):.8f} ref {float(ref):.8f} grad rel-L2 {err_g:.3e} "
          f"D {got_d!r} ref {D!r}")
    torch.testing.assert_close(loss[0].double(), ref, rtol=1e-5, atol=1e-5)
    assert err_g < 1e-2
    assert (dl[:R, V:].float() == 0).all()  # pad columns
    zero_rows = (pw[torch.arange(R, device=DEV) % T] == 0) if pw is not None else None
    if zero_rows is not None:
        assert int(zero_rows.sum()) > 0
        assert (dl[:R][zero_rows].float() == 0).all()
        assert V == 1 or (dl[:R][~zero_rows][:, :V].float() != 0).any()  # (V = 1: the gradient is zero everywhere)
    assert (dl[R:].float() == 7.0).all()  # the rows behind the problem
    if cw is None and pw is None:
        assert got_d == -1.0  # eps alone: no pre-pass, D = R exactly
    else:
        assert abs(got_d - D) <= 1e-12 * D


@pytest.mark.parametrize("R,T,V", [(77, 7, 2), (4100, 100, 65), (9000, 125, 1500)])
def test_block_shares_give_the_same_bits_run_to_run(R, T, V):
    x, t, w, u = _inputs(R, T, V)
    a = _run(x, t, T, 0.1, w, u, part=True)
    b = _run(x, t, T, 0.1, w, u, part=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))
    assert torch.equal(a[2].view(torch.int64), b[2].view(torch.int64))
    torch.testing.assert_close(a[0][0].double(), loss_ref.objective(x, t, T, 0.1, w, u), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("R,T,V", [(33, 11, 5), (4100, 41, 900), (9000, 125, 1500)])
def test_neutral_arguments_match_the_plain_kernel(R, T, V):
    x, t, _, _ = _inputs(R, T, V)
    loss, dl, denom, _ = _run(x, t, T, 0.0, None, None)
    ld = r8(V)
    dl0 = torch.full((R, ld), 7.0, dtype=torch.bfloat16, device=DEV)
    loss0 = torch.zeros(1, device=DEV)
    assert ML.lib().mmt_op_cross_entropy(ML.stream_ptr(), R, V, ML.ptr(x), ML.ptr(t), ML.ptr(dl0), ld, ML.ptr(loss0)) == 0
    torch.cuda.synchronize()
    torch.testing.assert_close(loss[0], loss0[0], rtol=1e-5, atol=1e-5)
    assert rel(dl[:R].double(), dl0.double()) < 1e-2
    # ... and so do unit weights, with D = R from the pre-pass
    loss1, dl1, denom1, _ = _run(x, t, T, 0.0, torch.ones(V, device=DEV), torch.ones(T, device=DEV))
    assert float(denom1[0]) == R
    torch.testing.assert_close(loss1[0], loss0[0], rtol=1e-5, atol=1e-5)
    assert rel(dl1[:R].double(), dl0.double()) < 1e-2


def test_zero_denominator_gives_nan_and_raises_both_flag_words():
    R, T, V = 77, 11, 13
    x, _, _, _ = _inputs(R, T, V)
    t = torch.randint(0, 6, (R,), generator=torch.Generator().manual_seed(3)).to(DEV)
    w = torch.ones(V, device=DEV)
    w[:6] = 0  # every class that occurs
    loss, _, denom, flag = _run(x, t, T, 0.0, w, None, part=True, flag=True)
    assert float(denom[0]) == 0.0
    assert math.isnan(float(loss[0]))
    assert flag.tolist() == [1, 1]
    # a healthy spec leaves the flag alone
    w[:6] = 1
    loss, _, _, flag = _run(x, t, T, 0.1, w, None, part=True, flag=True)
    assert math.isfinite(float(loss[0])) and flag.tolist() == [0, 0]
