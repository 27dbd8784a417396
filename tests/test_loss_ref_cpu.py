"""tests/loss_ref.py against torch's own cross-entropy, in fp64 on the CPU: the reference the GPU tests of the
training objective compare with is itself checked here."""
import math

import pytest
import torch
import torch.nn.functional as F

import loss_ref

CASES = [(33, 11, 5), (77, 7, 13), (64, 16, 2), (40, 8, 1), (120, 24, 144)]


def _case(R, T, V, seed=0):
    g = torch.Generator().manual_seed(1000 * R + V + seed)
    x = torch.randn(R, V, generator=g, dtype=torch.float64) * 2
    t = torch.randint(0, V, (R,), generator=g)
    w = torch.rand(V, generator=g, dtype=torch.float64) + 0.2
    u = torch.rand(T, generator=g, dtype=torch.float64)
    u[: T // 4] = 0
    return x, t, w, u


@pytest.mark.parametrize("R,T,V", CASES)
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_equals_torch_with_unit_position_weights(R, T, V, eps):
    x, t, w, _ = _case(R, T, V)
    for weight in (None, w):
        rows = F.cross_entropy(x, t, weight=weight, label_smoothing=eps, reduction="none")
        torch.testing.assert_close(loss_ref.row_losses(x, t, eps, weight), rows, rtol=1e-13, atol=1e-13)
        mean = F.cross_entropy(x, t, weight=weight, label_smoothing=eps)
        torch.testing.assert_close(loss_ref.objective(x, t, T, eps, weight, None), mean, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("R,T,V", CASES)
def test_neutral_spec_is_plain_cross_entropy(R, T, V):
    x, t, _, _ = _case(R, T, V)
    torch.testing.assert_close(loss_ref.objective(x, t, T), F.cross_entropy(x, t), rtol=1e-14, atol=1e-14)
    torch.testing.assert_close(loss_ref.objective(x, t, T, 0.0, torch.ones(V), torch.ones(T)), F.cross_entropy(x, t),
                               rtol=1e-14, atol=1e-14)
    assert float(loss_ref.denominator(t, T)) == R


@pytest.mark.parametrize("R,T,V", CASES)
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_closed_form_gradient_equals_autograd(R, T, V, eps):
    x, t, w, u = _case(R, T, V)
    for weight, pos in ((None, None), (w, None), (None, u), (w, u)):
        xr = x.clone().requires_grad_(True)
        loss_ref.objective(xr, t, T, eps, weight, pos).backward()
        torch.testing.assert_close(loss_ref.gradient(x, t, T, eps, weight, pos), xr.grad, rtol=1e-12, atol=1e-14)
        # ... and torch's own objective where it has one
        if pos is None:
            xt = x.clone().requires_grad_(True)
            F.cross_entropy(xt, t, weight=weight, label_smoothing=eps).backward()
            torch.testing.assert_close(xr.grad, xt.grad, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("R,T,V", CASES)
def test_zero_position_weights_equal_torch_on_the_remaining_rows(R, T, V):
    x, t, w, _ = _case(R, T, V)
    u = torch.ones(T, dtype=torch.float64)
    u[: T // 3 + 1] = 0
    keep = u[torch.arange(R) % T] > 0
    ref = F.cross_entropy(x[keep], t[keep], weight=w, label_smoothing=0.1)
    torch.testing.assert_close(loss_ref.objective(x, t, T, 0.1, w, u), ref, rtol=1e-13, atol=1e-13)
    g = loss_ref.gradient(x, t, T, 0.1, w, u)
    assert (g[~keep] == 0).all()
    torch.testing.assert_close(loss_ref.denominator(t, T, w, u), w[t[keep]].sum(), rtol=1e-14, atol=0)


def test_zero_denominator_is_nan_as_in_torch():
    x, t, w, u = _case(33, 11, 5)
    w = torch.ones(5, dtype=torch.float64)
    w[t.unique()] = 0  # every class that occurs
    if bool((w == 0).all()):
        w = torch.zeros(5, dtype=torch.float64)
    assert math.isnan(float(F.cross_entropy(x, t, weight=w)))
    assert math.isnan(float(loss_ref.objective(x, t, 11, 0.0, w, None)))
    assert float(loss_ref.denominator(t, 11, w, None)) == 0.0
