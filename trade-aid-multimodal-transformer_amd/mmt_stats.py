"""Per-tensor gradient / parameter statistics and the first-fault record (include/mmt.h: mmt_tensor_stats).

    stats = TensorStats(model, mode="skipped")            # or "every"
    opt = mmt_optim.AdamW(model.parameters(), lr, skip_nonfinite=True, stats=stats)
    ...                                                   # train; step() enqueues the statistics, no sync
    rep = stats.read()                                    # where the loop syncs anyway: one D2H copy
    if rep is not None:
        print(rep.format())

Mode "every" overwrites the record at every optimizer step. Mode "skipped" arms a latch: the device writes
the record at the first step the guard skips (non-finite gradient norm) and keeps it, whatever follows, until
`read(rearm=True)` re-arms it; a clean step costs three launches that return after one load each.

The segment table comes from the model's reference tensors (`model.tensor_segments()`). The tensors are
padded apart in the flat buffer, so every gap gets a segment of its own in the table the device sees
(include/mmt.h); the report drops those again. All of it is opt-in: nothing here runs unless asked for.
"""
import ctypes
import math

import numpy as np
import torch

import mmt_lib as ML

MODES = ("skipped", "every")


def build_segments(names, begins, ends):
    """The device's segment table for named tensors [begin, end) in offset order: (bounds, named) where
    `bounds` is the ascending offset list (len = segments + 1) with every gap between two tensors as a
    segment of its own, and named[i] is the index in that table of tensor i. Raises ValueError for tensors
    that are unsorted, overlap, or have end < begin."""
    if not (len(names) == len(begins) == len(ends)):
        raise ValueError("names, begins and ends must have one entry per tensor")
    bounds, named = [], []
    for name, b, e in zip(names, begins, ends):
        b, e = int(b), int(e)
        if b < 0 or e < b:
            raise ValueError(f"tensor {name!r}: bad range [{b}, {e})")
        if bounds and b < bounds[-1]:
            raise ValueError(f"tensor {name!r} at [{b}, {e}) overlaps or precedes the tensor before it "
                             f"(which ends at {bounds[-1]}): the segments must be sorted and disjoint")
        if not bounds:
            bounds.append(b)
        elif b > bounds[-1]:
            bounds.append(b)  # the gap before this tensor: an unnamed segment
        named.append(len(bounds) - 1)
        bounds.append(e)
    if not bounds:
        bounds = [0]
    return bounds, named


class StatsReport:
    """One snapshot, on the host. Arrays are numpy, one entry per named tensor, in offset order."""

    def __init__(self, names, sqsum, absmax, nan_count, inf_count, first_bad, applied_steps=0, skipped_steps=0,
                 begins=None, stage_ranges=None):
        self.names = list(names)
        self.sqsum = np.asarray(sqsum, dtype=np.float64)
        self.absmax = np.asarray(absmax, dtype=np.float32)
        self.nan_count = np.asarray(nan_count, dtype=np.int64)
        self.inf_count = np.asarray(inf_count, dtype=np.int64)
        self.first_bad = np.asarray(first_bad, dtype=np.int64)
        self.applied_steps = int(applied_steps)
        self.skipped_steps = int(skipped_steps)
        self.begins = None if begins is None else [int(b) for b in begins]
        self.stage_ranges = None if stage_ranges is None else [(int(b), int(e)) for b, e in stage_ranges]
        self._index = {n: i for i, n in enumerate(self.names)}

    @classmethod
    def from_record(cls, raw, names, named, begins=None, stage_ranges=None):
        """From the bytes of a device record (header + mmt_tensor_stat per table segment); `named` picks the
        table entries of the named tensors. None when the record holds no snapshot."""
        raw = bytes(raw)
        hdr = ML.MmtStatsHeader.from_buffer_copy(raw[:ctypes.sizeof(ML.MmtStatsHeader)])
        if hdr.valid == 0:
            return None
        dt = np.dtype([("sqsum", "<f8"), ("nan_count", "<i8"), ("inf_count", "<i8"), ("first_bad", "<i8"),
                       ("absmax", "<f4"), ("reserved", "<f4")])
        assert dt.itemsize == ctypes.sizeof(ML.MmtTensorStat)
        st = np.frombuffer(raw, dtype=dt, count=hdr.nseg, offset=ctypes.sizeof(ML.MmtStatsHeader))
        sel = st[np.asarray(named, dtype=np.int64)] if len(named) else st[:0]
        return cls(names, sel["sqsum"], sel["absmax"], sel["nan_count"], sel["inf_count"], sel["first_bad"],
                   hdr.applied_steps, hdr.skipped_steps, begins, stage_ranges)

    # ------------------------------------------------------------------ per tensor
    def norm(self, name):
        """L2 norm of the finite elements of one tensor."""
        return math.sqrt(float(self.sqsum[self._index[name]]))

    @property
    def global_norm(self):
        """L2 norm over all named tensors; NaN when any element is non-finite (as the guard's norm is)."""
        if self.nan_count.sum() or self.inf_count.sum():
            return float("nan")
        return math.sqrt(float(self.sqsum.sum()))

    def nonfinite(self):
        """[(name, nan_count, inf_count, first_bad)] of the tensors that hold a NaN or an infinity."""
        bad = np.nonzero((self.nan_count > 0) | (self.inf_count > 0))[0]
        return [(self.names[i], int(self.nan_count[i]), int(self.inf_count[i]), int(self.first_bad[i])) for i in bad]

    def largest(self, k=3):
        """[(name, norm)] of the k tensors with the largest norms."""
        order = np.argsort(-self.sqsum, kind="stable")[:k]
        return [(self.names[i], math.sqrt(float(self.sqsum[i]))) for i in order]

    # ------------------------------------------------------------------ per backward stage
    def _stage_of(self):
        if self.begins is None or self.stage_ranges is None:
            raise ValueError("this report has no stage ranges (begins / stage_ranges)")
        out = []
        for b in self.begins:
            out.append(next((s for s, (lo, hi) in enumerate(self.stage_ranges) if lo <= b < hi), -1))
        return out

    def by_stage(self):
        """One dict per backward stage, in execution order (post block, layers L-1 .. 0, embeddings):
        stage, begin, end, tensors, nonfinite (tensors holding a NaN / Inf) and norm (finite elements)."""
        stage_of = np.asarray(self._stage_of(), dtype=np.int64)
        bad = (self.nan_count > 0) | (self.inf_count > 0)
        out = []
        for s, (lo, hi) in enumerate(self.stage_ranges):
            sel = stage_of == s
            out.append({"stage": s, "begin": lo, "end": hi, "tensors": int(sel.sum()),
                        "nonfinite": int((sel & bad).sum()), "norm": math.sqrt(float(self.sqsum[sel].sum()))})
        return out

    @property
    def first_poisoned_stage(self):
        """The earliest stage in backward order that holds a non-finite tensor (where the fault entered: every
        later stage consumes its gradients), or None."""
        for st in self.by_stage():
            if st["nonfinite"]:
                return st["stage"]
        return None

    def format(self, max_names=8):
        """One line. After a fault: the step, the count of non-finite tensors, the first poisoned stage and up
        to max_names tensors with their NaN / Inf counts; otherwise the global norm and the three largest
        per-tensor norms."""
        bad = self.nonfinite()
        head = f"applied {self.applied_steps} skipped {self.skipped_steps}"
        if bad:
            stage = "n/a"
            if self.begins is not None and self.stage_ranges is not None:
                fp = self.first_poisoned_stage
                stage = "n/a" if fp is None else f"{fp}/{len(self.stage_ranges)}"
            shown = ", ".join(f"{n} (nan {a}, inf {b}, first at {f})" for n, a, b, f in bad[:max_names])
            more = f", +{len(bad) - max_names} more" if len(bad) > max_names else ""
            return (f"{head} | non-finite tensors: {len(bad)}/{len(self.names)} | first poisoned stage: {stage} | "
                    f"{shown}{more}")
        top = ", ".join(f"{n} {v:.4g}" for n, v in self.largest(3))
        return f"{head} | norm: {self.global_norm:.4f} | tensors: {len(self.names)} | largest: {top}"


class TensorStats:
    """Device record + scratch for the statistics of one model's flat buffers (gradients or parameters: the
    same layout). `record()` only enqueues; `read()` is the one call that copies to the host."""

    def __init__(self, model, mode="skipped"):
        if mode not in MODES:
            raise ValueError(f"TensorStats mode must be one of {MODES}, got {mode!r}")
        self.model = model
        self.mode = mode
        self._rec = self._scratch = None
        if model.flat_params.is_cuda:
            self._prepare()

    def _prepare(self):
        m = self.model
        seg = m.tensor_segments()
        dev = m.flat_params.device
        L = ML.lib()
        self._seg = seg
        self._nseg = len(seg["bounds"]) - 1
        self._n = m.flat_params.numel()
        self._rec = torch.zeros(L.mmt_stats_record_bytes(self._nseg), dtype=torch.uint8, device=dev)
        self._scratch = torch.empty(L.mmt_stats_scratch_bytes(self._n, self._nseg), dtype=torch.uint8, device=dev)
        self._stages = m.backward_stage_ranges()

    def record(self, buf, guard=None):
        """Enqueue the statistics of `buf` (a flat fp32 device tensor with the layout of flat_params) on the
        current stream. Mode "every": always; mode "skipped": only if `guard` (the optimizer's device guard
        state, after mmt_guard_finalize) says that this step is skipped and the record is still armed."""
        if self._rec is None:
            self._prepare()
        if self.mode == "skipped" and guard is None:
            raise ValueError("TensorStats mode 'skipped' needs the optimizer's guard state")
        if buf.numel() != self._n or not buf.is_contiguous():
            raise ValueError("TensorStats.record needs a contiguous buffer with the layout of flat_params")
        if buf.dtype != torch.float32 or buf.device != self._rec.device:
            raise ValueError("TensorStats.record needs an fp32 buffer on the model's device")
        mode = ML.STATS_ON_SKIP if self.mode == "skipped" else ML.STATS_ALWAYS
        with torch.cuda.device(buf.device):
            rc = ML.lib().mmt_tensor_stats(ML.stream_ptr(buf.device), ML.ptr(buf), self._n, ML.ptr(self._seg["device"]),
                                           self._nseg, mode, ML.ptr(guard), ML.ptr(self._scratch), ML.ptr(self._rec))
        ML.check(rc, None, "mmt_tensor_stats")

    def read(self, rearm=True):
        """The record as a StatsReport (one D2H copy; syncs), or None while it is empty. rearm=True clears
        `valid` on the device afterwards (a 4-byte memset on the current stream), so the next skipped step
        (mode "skipped") is recorded again."""
        if self._rec is None:
            return None
        raw = self._rec.cpu().numpy().tobytes()
        seg = self._seg
        rep = StatsReport.from_record(raw, seg["names"], seg["named"], seg["begins"], self._stages)
        if rep is not None and rearm:
            self._rec[0:4].zero_()
        return rep
