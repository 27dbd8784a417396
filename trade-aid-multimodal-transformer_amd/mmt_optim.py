"""Fused AdamW on the gfx950 library — drop-in for torch.optim.AdamW(m.parameters(), lr=...)
(reference main.py:464, 648-650).

Semantics follow torch's AdamW defaults: betas (0.9, 0.999), eps 1e-8, weight_decay 0.01,
decoupled decay, bias correction; parameters whose .grad is None are skipped entirely (the
model's `flat_unused`, the CrossAttention parameters that never get a gradient). The stock
torch.optim.AdamW gives the same result on the model (tests/test_gpu_model.py); this one runs the
update as one fused HIP kernel over the flat buffer.

Guarded step (opt-in: `max_grad_norm` and / or `skip_nonfinite`; include/mmt.h). With either set,
step() computes the global gradient norm over every parameter of every group on the device
(mmt_grad_sqsum per tensor, fp64, fixed order), derives torch's clip_grad_norm_ coefficient
min(1, max_grad_norm / (norm + 1e-6)) and the non-finite verdict in one tiny launch
(mmt_guard_finalize) and applies AdamW to grads * coef (mmt_adamw_step_guarded), or to nothing at all
when the norm is NaN / Inf and skip_nonfinite is set. Nothing is copied to the host and nothing syncs:
the step count lives on the device (as in torch's capturable AdamW), so a skipped step does not advance
the bias correction. `last_grad_norm` is a 0-dim device tensor; `counters()` is the only call that syncs.
With both options at their defaults step() is the plain path above, unchanged.

Statistics (opt-in: `stats=mmt_stats.TensorStats(model, mode)`). step() enqueues the per-tensor statistics of
the gradient of that model's `flat_params`: on the guarded path between mmt_guard_finalize and the first
guarded step (mode "skipped": only the first step the guard skips is recorded, on the device, until the
record is re-armed; mode "every": every step), on the plain path before the step (mode "every" only). Still
no copy to the host and no sync: `stats.read()` is the call that syncs.
"""
import math

import torch

import mmt_lib as ML

_HDR_COUNTERS = (16, 40)  # byte range of applied / skipped / clipped steps in struct mmt_guard_header


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 skip_nonfinite=False, stats=None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)):
                raise TypeError(f"max_grad_norm must be a positive number or None, got {max_grad_norm!r}")
            if math.isnan(max_grad_norm) or max_grad_norm <= 0.0:
                raise ValueError(f"max_grad_norm must be a positive number or None, got {max_grad_norm!r}")
        if not isinstance(skip_nonfinite, bool):
            raise TypeError(f"skip_nonfinite must be a bool, got {skip_nonfinite!r}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = skip_nonfinite
        self.guarded = self.max_grad_norm is not None or skip_nonfinite
        if stats is not None:
            if getattr(stats, "mode", None) not in ("skipped", "every") or not callable(getattr(stats, "record", None)):
                raise TypeError(f"stats must be an mmt_stats.TensorStats or None, got {stats!r}")
            if stats.mode == "skipped" and not self.guarded:
                raise ValueError("stats in mode 'skipped' records the first step the guard skips: it needs a "
                                 "guarded optimizer (skip_nonfinite=True; mode 'every' runs on any optimizer)")
        self.stats = stats
        if self.guarded:
            self._check_betas()
        self._guard = None          # device guard state (mmt_guard_state_bytes), made at the first guarded step
        self._loaded_applied = None  # applied count of a loaded state_dict, written into the next guard state

    @torch.no_grad()
    def step(self, closure=None):
        if self.guarded:
            return self._step_guarded(closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = ML.lib()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.device.type != "cuda" or p.dtype != torch.float32:
                    raise RuntimeError("mmt AdamW runs on fp32 ROCm tensors only (no CPU path)")
                g = p.grad
                if not g.is_contiguous() or not p.is_contiguous():
                    raise RuntimeError("mmt AdamW needs contiguous params/grads")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                n = p.numel()
                if self.stats is not None and p is self.stats.model.flat_params:
                    self.stats.record(g)
                rc = L.mmt_adamw_step(None, ML.stream_ptr(p.device), ML.ptr(p), ML.ptr(g), ML.ptr(st["exp_avg"]),
                                      ML.ptr(st["exp_avg_sq"]), n, st["step"], group["lr"], b1, b2, group["eps"],
                                      group["weight_decay"])
                ML.check(rc, None, "mmt_adamw_step")
        return loss

    # ------------------------------------------------------------------ guarded step
    def _check_betas(self):
        """One device step count and one pair of bias corrections: every group needs the same betas
        (checked at construction and at every guarded step: groups can be added or edited later)."""
        if len({tuple(g["betas"]) for g in self.param_groups}) != 1:
            raise ValueError("a guarded AdamW keeps one device step count: every group needs the same betas")

    def _guard_state(self, device):
        if self._guard is None:
            self._guard = torch.zeros(ML.lib().mmt_guard_state_bytes(), dtype=torch.uint8, device=device)
            if self._loaded_applied:
                self._guard[_HDR_COUNTERS[0]:_HDR_COUNTERS[0] + 8].view(torch.int64).fill_(self._loaded_applied)
            self._loaded_applied = None
        elif self._guard.device != device:
            raise RuntimeError("a guarded mmt AdamW keeps all its parameters on one device")
        return self._guard

    def _step_guarded(self, closure):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_betas()
        work = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.device.type != "cuda" or p.dtype != torch.float32:
                    raise RuntimeError("mmt AdamW runs on fp32 ROCm tensors only (no CPU path)")
                if not p.grad.is_contiguous() or not p.is_contiguous():
                    raise RuntimeError("mmt AdamW needs contiguous params/grads")
                work.append((group, p))
        if not work:
            return loss
        L = ML.lib()
        dev = work[0][1].device
        guard = self._guard_state(dev)
        gp = ML.ptr(guard)
        applied = guard[_HDR_COUNTERS[0]:_HDR_COUNTERS[0] + 8].view(torch.int64)[0]
        b1, b2 = work[0][0]["betas"]
        with torch.cuda.device(dev):
            s = ML.stream_ptr(dev)
            for k, (group, p) in enumerate(work):
                if p.device != dev:
                    raise RuntimeError("a guarded mmt AdamW keeps all its parameters on one device")
                ML.check(L.mmt_grad_sqsum(s, ML.ptr(p.grad), p.numel(), 1 if k else 0, gp), None, "mmt_grad_sqsum")
            max_norm = self.max_grad_norm if self.max_grad_norm is not None else 0.0
            ML.check(L.mmt_guard_finalize(s, max_norm, 1 if self.skip_nonfinite else 0, b1, b2, gp), None,
                     "mmt_guard_finalize")
            if self.stats is not None:  # the verdict is in, the gradients are still intact
                for group, p in work:
                    if p is self.stats.model.flat_params:
                        self.stats.record(p.grad, guard)
            for group, p in work:
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] = applied  # the device count (a view of the guard header)
                rc = L.mmt_adamw_step_guarded(None, s, ML.ptr(p), ML.ptr(p.grad), ML.ptr(st["exp_avg"]),
                                              ML.ptr(st["exp_avg_sq"]), p.numel(), group["lr"], b1, b2, group["eps"],
                                              group["weight_decay"], gp)
                ML.check(rc, None, "mmt_adamw_step_guarded")
        return loss

    @property
    def last_grad_norm(self):
        """Global gradient norm of the last guarded step (before clipping): a 0-dim fp32 device tensor that
        views the guard header (no copy, no sync); None before the first guarded step."""
        if self._guard is None:
            return None
        return self._guard[0:4].view(torch.float32)[0]

    def counters(self):
        """(applied, skipped, clipped) steps of the guarded optimizer as Python ints. Syncs."""
        if self._guard is None:
            return (int(self._loaded_applied or 0), 0, 0)
        a, s, c = self._guard[_HDR_COUNTERS[0]:_HDR_COUNTERS[1]].view(torch.int64).tolist()
        return (a, s, c)

    def state_dict(self):
        """torch's state_dict; a guarded optimizer's device step count is materialised as a Python int
        (state["step"] = the applied count; one sync)."""
        sd = super().state_dict()
        if self.guarded:
            applied = None
            for k, st in sd["state"].items():
                if torch.is_tensor(st.get("step")):
                    if applied is None:
                        applied = self.counters()[0]
                    # a copy: torch hands out the live per-parameter dicts, whose "step" stays the device view
                    sd["state"][k] = dict(st, step=applied)
        return sd

    def load_state_dict(self, state_dict):
        """torch's load_state_dict; a guarded optimizer takes state["step"] as an int (the applied count,
        one value for the whole optimizer) and puts it back on the device."""
        super().load_state_dict(state_dict)
        if not self.guarded:
            return
        steps = {int(st["step"]) for st in self.state.values() if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"a guarded AdamW keeps one step count for all parameters, the state has {sorted(steps)}")
        applied = steps.pop() if steps else 0
        if self._guard is not None:
            self._guard[_HDR_COUNTERS[0]:_HDR_COUNTERS[0] + 8].view(torch.int64).fill_(applied)
        else:
            self._loaded_applied = applied
