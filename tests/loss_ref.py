"""fp64 reference of the training objective (include/mmt.h, mmt_set_loss): label smoothing eps, class weights
w [V], position weights u [T] on logits x [R, V] whose row r sits at position r mod T.

    row_r = (1 - eps) w[t_r] (lse_r - x[r, t_r]) + eps / V * sum_c w[c] (lse_r - x[r, c])
    D     = sum_r u[r mod T] w[t_r]
    loss  = sum_r u[r mod T] row_r / D
    dloss / dx[r, j] = u_r / D (p[r, j] ((1 - eps) w[t_r] + eps Wbar) - (1 - eps) w[t_r] [j == t_r] - eps / V w[j])

`objective` is written with differentiable torch ops (autograd goes through it), `gradient` is the closed form.
"""
import torch


def _vectors(x, T, w, u):
    R, V = x.shape
    w = torch.ones(V, dtype=torch.float64, device=x.device) if w is None else w.to(x.device, torch.float64)
    u = torch.ones(T, dtype=torch.float64, device=x.device) if u is None else u.to(x.device, torch.float64)
    ur = u[torch.arange(R, device=x.device) % T]
    return w, ur


def row_losses(x, t, eps=0.0, w=None):
    """[R] fp64: F.cross_entropy(x, t, weight=w, label_smoothing=eps, reduction="none")."""
    x = x.to(torch.float64)
    R, V = x.shape
    w, _ = _vectors(x, 1, w, None)
    nlp = torch.logsumexp(x, dim=1, keepdim=True) - x  # lse - x[c] >= 0
    hard = w[t] * nlp.gather(1, t.view(R, 1)).squeeze(1)
    if eps == 0.0:
        return hard
    return (1.0 - eps) * hard + (eps / V) * (nlp * w[None, :]).sum(1)


def denominator(t, T, w=None, u=None, V=None):
    """D = sum_r u[r mod T] w[t_r] in fp64."""
    R = t.numel()
    ur = torch.ones(R, dtype=torch.float64) if u is None else u.to("cpu", torch.float64)[torch.arange(R) % T]
    wt = torch.ones(R, dtype=torch.float64) if w is None else w.to("cpu", torch.float64)[t.cpu()]
    return (ur * wt).sum()


def objective(x, t, T, eps=0.0, w=None, u=None):
    """The loss, fp64 scalar (NaN for D == 0, as torch's weighted mean)."""
    x = x.to(torch.float64)
    wv, ur = _vectors(x, T, w, u)
    D = (ur * wv[t]).sum()
    return (ur * row_losses(x, t, eps, w)).sum() / D


def gradient(x, t, T, eps=0.0, w=None, u=None):
    """dloss / dx [R, V] fp64 by the closed form."""
    x = x.to(torch.float64)
    R, V = x.shape
    wv, ur = _vectors(x, T, w, u)
    wt = wv[t]
    D = (ur * wt).sum()
    p = torch.softmax(x, dim=1)
    g = p * ((1.0 - eps) * wt + eps * wv.sum() / V)[:, None] - (eps / V) * wv[None, :]
    g[torch.arange(R, device=x.device), t] -= (1.0 - eps) * wt
    return g * (ur / D)[:, None]
