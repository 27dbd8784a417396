"""model.py — drop-in `MultimodalTransformer` backed by the gfx950 HIP library (libmmt_hip.so).

Same constructor, forward signature, state_dict keys/shapes and train()/eval() behaviour as the
reference (model.py:355-402 of tsnuk/trade-AId-multimodal-transformer):

    m = MultimodalTransformer(num_modalities, vocab_sizes, all_modality_params).to("cuda")
    logits_list, losses_list = m(idx_list, targets_list)
    sum(losses_list).backward()

Differences that are by design:
  * all parameters that receive gradients live in ONE flat fp32 `nn.Parameter` (`flat_params`);
    the parameters of a CrossAttention with no KV modality (M == 1, reference model.py:198-200,
    238), which never get a gradient, live in a second one (`flat_unused`) whose `.grad` stays
    None, so the reference's stock `torch.optim.AdamW(m.parameters(), lr)` (main.py:464) skips
    them exactly as it does in the reference. `state_dict()` / `load_state_dict()` expose and
    accept exactly the reference's per-head keys (including the `.tril` buffers, emitted as one
    shared tensor), so reference checkpoints round-trip;
  * compute runs in bf16 on MFMA with fp32 accumulation, fp32 master weights/residual stream;
  * forward/backward run only on a ROCm device (there is no CPU path: the CPU oracle lives in
    oracle/ and is test infrastructure only);
  * logits are outputs without autograd history (the reference training loop differentiates
    only the losses; main.py:646-649);
  * training batches are exactly block_size long (as the reference's get_batch makes them); a
    shorter sequence without targets (generate, inference) runs right-padded to block_size: the
    attention is causal, so the logits of the real positions are exactly those of the short run;
  * generate keeps a KV cache (one prefill forward, then one position per token through
    mmt_decode_step) while the sequence fits the block; the reference re-runs the forward.
"""
import contextlib
import ctypes

import torch
import torch.nn as nn

import mmt_lib as ML
import mmt_rollout as MR
from config_utils import (_get_block_size, _get_deterministic, _get_dropout, _get_n_embd, _get_n_head, _get_n_layer,
                          _get_precision)
from mmt_rollout import (DEFAULT_QUANTILES, EVIDENCE_MODES, GENERATED, GIVEN, HELD, JointPlan,  # noqa: F401
                         check_forecast, check_horizon, check_num_samples, joint_setting, plan_joint, resample_points,
                         tile_prompts)


class _MmtStep(torch.autograd.Function):
    """One forward through the C-ABI; its backward is mmt_backward into a fresh flat grad (or, with
    set_grad_accumulation on, in place into flat_params.grad: then no gradient is returned for `flat`)."""

    @staticmethod
    def forward(ctx, flat, owner, training, n_mod, *tensors):
        idx = list(tensors[:n_mod])
        tgt = list(tensors[n_mod:]) if len(tensors) > n_mod else None
        logits, losses = owner._launch_forward(flat, idx, tgt, training)
        ctx.owner = owner
        ctx.gen = owner._gen
        ctx.keep = (idx, tgt)  # the engine reads the token ids again in the embedding backward
        ctx.n_tensors = len(tensors)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*logits)
        if losses is None:
            return tuple(logits)
        return (*logits, losses)

    @staticmethod
    def backward(ctx, *grads):
        g_losses = grads[-1]
        nones = (None,) * (3 + ctx.n_tensors)
        if g_losses is None:
            return nones
        owner = ctx.owner
        if owner._gen != ctx.gen:
            raise RuntimeError("MultimodalTransformer: backward of a stale forward (another forward ran in between); "
                               "the saved activations live in one workspace per model")
        grad = owner._launch_backward(g_losses)
        return (grad,) + nones


class MultimodalTransformer(nn.Module):
    """Reference model.py:355-402 (see module docstring)."""

    def __init__(self, num_modalities, vocab_sizes, all_modality_params):
        super().__init__()
        self.num_modalities = int(num_modalities)
        self.vocab_sizes = [int(v) for v in vocab_sizes]
        self.all_modality_params = all_modality_params
        M = self.num_modalities
        if not (1 <= M <= ML.MAX_MOD):
            raise ValueError("num_modalities must be 1..8")
        self.n_embd, self.n_head, self.n_layer = _get_n_embd(), _get_n_head(), _get_n_layer()
        self.block_size, self.dropout_p = _get_block_size(), float(_get_dropout())
        cfg = ML.MmtConfig()
        cfg.num_modalities = M
        cfg.n_embd, cfg.n_head, cfg.n_layer, cfg.block_size = self.n_embd, self.n_head, self.n_layer, self.block_size
        for i in range(M):
            cfg.vocab_sizes[i] = self.vocab_sizes[i]
            cfg.cross_attention[i] = 1 if all_modality_params[i][8] else 0  # model.py:196
        cfg.dropout = self.dropout_p
        cfg.seed = 0
        self.precision = _get_precision()
        cfg.precision = 1 if self.precision == "fp8" else 0
        L = ML.lib()
        ctx = L.mmt_create(ctypes.byref(cfg))
        if not ctx:
            raise ML.MmtError("mmt_create failed: " + L.mmt_create_error().decode())
        self._ctx = ctypes.c_void_p(ctx)
        self.deterministic = False
        self.set_deterministic(_get_deterministic())
        n = L.mmt_param_count(self._ctx)
        self._n_active = L.mmt_param_active_count(self._ctx)
        self._tensors = []
        name = ctypes.create_string_buffer(256)
        off, nd, shape, kind = ML.c_i64(), ML.c_i32(), (ML.c_i64 * 2)(), ML.c_i32()
        for i in range(L.mmt_tensor_count(self._ctx)):
            ML.check(L.mmt_tensor_info(self._ctx, i, name, 256, ctypes.byref(off), ctypes.byref(nd), shape,
                                       ctypes.byref(kind)), self._ctx, "mmt_tensor_info")
            shp = tuple(shape[d] for d in range(nd.value))
            self._tensors.append((name.value.decode(), off.value, shp, kind.value))
        self._tril_keys = self._make_tril_keys()
        flat = torch.zeros(n, dtype=torch.float32)
        self._init_flat(flat)
        na = self._n_active
        self.flat_params = nn.Parameter(flat[:na].clone())
        # never-used CrossAttention parameters (M == 1): their own Parameter, .grad stays None
        self.flat_unused = nn.Parameter(flat[na:].clone()) if n > na else None
        self._dropout_counter = 0
        self._dp_rank = 0  # data-parallel rank (mmt_dist.enable_data_parallel): folded into the dropout seed
        self._sticky_carry = 0  # sticky non-finite bits of workspaces replaced since the last clear
        self._ws = None
        self._ws_batch = -1
        self._ws_bytes = {}
        self._fan = None  # the fan buffer of _decode_fanout_step
        self.last_generate_path = None  # generate(num_samples=...): "fanout" or "tiled", whichever ran last
        self.calibrated_temperatures = {}  # set_calibrated_temperatures: what temperature="calibrated" stands for
        self._gen = 0
        self._last = None
        self._grad_sync = None  # mmt_dist.GradSync when data parallel
        self.grad_accumulation = False  # set_grad_accumulation: the backward writes into flat_params.grad in place
        self._grad_buf = None  # the in-place mode's persistent gradient buffer (becomes .grad when .grad is None)
        self._no_sync = False  # inside no_sync(): no gradient exchange
        self._loss_host = None  # set_loss: [(eps, class weights, position weights)] on the host; None: the plain loss
        self._loss_dev = None   # ... and (device, the device tensors the engine reads), made at the first forward there

    def set_loss(self, label_smoothing=0.0, class_weights=None, position_weights=None):
        """The training objective (include/mmt.h, mmt_set_loss): torch's F.cross_entropy(weight=, label_smoothing=)
        extended by a weight per position of the window, for every forward that gets targets (train or eval mode).
        Each argument is one value for all modalities or a {modality: value} dict: label_smoothing a number in
        [0, 1), class_weights a vector [V_i], position_weights a vector [block_size], both finite, >= 0 and not all
        zero (ValueError otherwise, before anything changes). No arguments: back to the plain mean cross-entropy.
        The model keeps the device copies alive; the spec is a plain attribute, not part of state_dict."""
        import mmt_loss
        spec = mmt_loss.normalize_spec(label_smoothing, class_weights, position_weights, self.vocab_sizes,
                                       self.block_size)
        self._install_loss(spec, self.flat_params.device)

    def _install_loss(self, spec, dev):
        M = self.num_modalities
        arr = (ML.MmtLossSpec * M)()
        keep = []
        for i in range(M if spec is not None else 0):
            eps, cw, pw = spec[i]
            cw = None if cw is None else cw.to(dev)
            pw = None if pw is None else pw.to(dev)
            keep.append((cw, pw))
            arr[i].label_smoothing = eps
            arr[i].class_weight = None if cw is None else cw.data_ptr()
            arr[i].position_weight = None if pw is None else pw.data_ptr()
        ML.check(ML.lib().mmt_set_loss(self._ctx, arr if spec is not None else None), self._ctx, "mmt_set_loss")
        self._loss_host = spec
        self._loss_dev = (dev, keep) if spec is not None else None

    @property
    def loss_spec(self):
        """The current objective: one {"label_smoothing", "class_weights", "position_weights"} dict per modality
        (host copies; None for absent weights), or None for the plain loss."""
        if self._loss_host is None:
            return None
        return [{"label_smoothing": e, "class_weights": None if w is None else w.clone(),
                 "position_weights": None if u is None else u.clone()} for e, w, u in self._loss_host]

    def set_calibrated_temperatures(self, mapping):
        """The per-head temperatures generate(temperature="calibrated") stands for: {modality: tau}, ints 0..M - 1
        and finite tau > 0 (ValueError otherwise); None clears them. estimate_loss with eval_temperature: fit stores
        the val fit here. A plain attribute (`calibrated_temperatures`): no parameter, no buffer, not in
        state_dict."""
        self.calibrated_temperatures = MR.check_calibrated_temperatures(mapping, self.num_modalities)

    def set_deterministic(self, on):
        """Deterministic training mode (include/mmt.h, mmt_set_deterministic): bit-identical gradients
        for identical inputs, parameters and dropout seed. Applies from the next forward on (a forward
        and its backward always run under one setting)."""
        ML.check(ML.lib().mmt_set_deterministic(self._ctx, 1 if on else 0), self._ctx, "mmt_set_deterministic")
        self.deterministic = bool(ML.lib().mmt_get_deterministic(self._ctx))

    # ------------------------------------------------------------------ layout / state_dict
    def _make_tril_keys(self):
        keys = []
        for l in range(self.n_layer):
            for i in range(self.num_modalities):
                for h in range(self.n_head):
                    keys.append(f"blocks.{l}.sa_layers.{i}.heads.{h}.tril")
            for i in range(self.num_modalities):
                if self.all_modality_params[i][8]:
                    for h in range(self.n_head):
                        keys.append(f"blocks.{l}.cross_attention_layers.{i}.heads.{h}.tril")
        return keys

    def _init_flat(self, flat):
        """model.py:372-378: Linear/Embedding weights N(0, 0.02), biases 0; LayerNorm 1 / 0."""
        for name, off, shp, kind in self._tensors:
            n = 1
            for s in shp:
                n *= s
            v = flat[off:off + n]
            if kind == 0:
                v.normal_(0.0, 0.02)
            elif kind == 2:
                v.fill_(1.0)
            else:
                v.zero_()

    def _view(self, off, shp, detach=False):
        """View of one reference tensor: a slice of flat_params, or of flat_unused past the
        active prefix."""
        n = 1
        for s in shp:
            n *= s
        if off >= self._n_active:
            base, off = self.flat_unused, off - self._n_active
        else:
            base = self.flat_params
        if detach:
            base = base.detach()
        return base[off:off + n].view(shp)

    def named_reference_tensors(self):
        """(reference state_dict key, view into flat_params) for every parameter."""
        for name, off, shp, _ in self._tensors:
            yield name, self._view(off, shp)

    def reference_grad_views(self):
        """(reference key, gradient view) for every parameter; None for the never-used ones."""
        g = self.flat_params.grad
        for name, off, shp, _ in self._tensors:
            if off >= self._n_active or g is None:
                yield name, None
                continue
            n = 1
            for s in shp:
                n *= s
            yield name, g[off:off + n].view(shp)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for name, off, shp, _ in self._tensors:
            destination[prefix + name] = self._view(off, shp, detach=not keep_vars)
        if self._tril_keys:
            T = self.block_size
            tril = torch.tril(torch.ones(T, T, device=self.flat_params.device))
            for k in self._tril_keys:
                destination[prefix + k] = tril  # one shared storage (saved once by torch.save)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        known = set()
        with torch.no_grad():
            for name, off, shp, _ in self._tensors:
                key = prefix + name
                known.add(key)
                if key not in state_dict:
                    missing_keys.append(key)
                    continue
                src = state_dict[key]
                if tuple(src.shape) != tuple(shp):
                    error_msgs.append(f"size mismatch for {key}: copying a param with shape {tuple(src.shape)}, "
                                      f"the shape in current model is {tuple(shp)}.")
                    continue
                self._view(off, shp, detach=True).copy_(src)
        T = self.block_size
        for k in self._tril_keys:
            key = prefix + k
            known.add(key)
            if key not in state_dict:
                missing_keys.append(key)
            elif tuple(state_dict[key].shape) != (T, T):
                error_msgs.append(f"size mismatch for {key}: {tuple(state_dict[key].shape)} vs {(T, T)}")
        if strict:
            for key in state_dict.keys():
                if key.startswith(prefix) and key not in known:
                    unexpected_keys.append(key)
        self._gen += 1

    # ------------------------------------------------------------------ execution
    def _workspace(self, B, device):
        if B not in self._ws_bytes:
            self._ws_bytes[B] = ML.lib().mmt_workspace_bytes(self._ctx, B)
            if self._ws_bytes[B] < 0:
                raise ML.MmtError("mmt_workspace_bytes failed")
        if self._ws is None or self._ws_batch != B or self._ws.device != device:
            off = ML.lib().mmt_loss_flag_offset(self._ctx, B)  # the same offset for every batch size
            if self._ws is not None:  # keep the sticky bits of the workspace being replaced
                self._sticky_carry |= int(self._ws[off + 4:off + 8].view(torch.int32).item())
            self._ws = None
            self._ws = torch.empty(self._ws_bytes[B], dtype=torch.uint8, device=device)
            self._ws_batch = B
            self._ws[off:off + 8].zero_()  # non-finite-loss flags (last forward, sticky)
        return self._ws

    def _launch_forward(self, flat, idx, tgt, training):
        L = ML.lib()
        dev = flat.device
        B, T = idx[0].shape
        ws = self._workspace(B, dev)
        logits = [torch.empty(B, T, V, dtype=torch.float32, device=dev) for V in self.vocab_sizes]
        losses = torch.empty(self.num_modalities, dtype=torch.float32, device=dev) if tgt is not None else None
        idx_arr = ML.ptr_array(idx)
        tgt_arr = ML.ptr_array(tgt) if tgt is not None else None
        if self._loss_dev is not None and self._loss_dev[0] != dev:
            self._install_loss(self._loss_host, dev)  # the model moved since set_loss: the weights follow it
        if training:
            self.last_dropout_seed = self._next_dropout_seed(dev)
            ML.check(L.mmt_set_dropout_seed(self._ctx, self.last_dropout_seed), self._ctx, "mmt_set_dropout_seed")
        with torch.cuda.device(dev):
            rc = L.mmt_forward(self._ctx, ML.stream_ptr(dev), B, idx_arr, tgt_arr, ML.ptr(flat), ML.ptr_array(logits),
                               ML.ptr(losses), ML.ptr(ws), 1 if training else 0)
        ML.check(rc, self._ctx, "mmt_forward")
        self._gen += 1
        self._last = (flat, idx, tgt)
        return logits, losses

    def _next_dropout_seed(self, dev):
        """Seed of this training step's dropout masks. The reference's nn.Dropout on a ROCm device
        draws from the device generator, never from torch's CPU generator (which get_batch's
        torch.randint start indices consume), so the seed is derived from the device generator's
        seed and Philox offset and the CPU random stream stays the reference's. The offset is
        bumped by a fixed 4 per forward only to keep the seed sequence repeatable under
        torch.manual_seed; this does NOT reproduce the reference's Philox consumption (its dropout
        calls advance the offset by tensor size), so later device-RNG users (e.g.
        torch.multinomial in generate) see a different stream than the reference's. Under data
        parallelism the rank is folded in: each rank draws its own masks."""
        self._dropout_counter += 1
        seed, off = 0, self._dropout_counter
        try:
            gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
            seed = int(gen.initial_seed())
            off = int(gen.get_offset())
            gen.set_offset(off + 4)
        except (AttributeError, RuntimeError, IndexError):
            pass
        x = (seed * 0x9E3779B97F4A7C15 + off * 0xBF58476D1CE4E5B9 + self._dropout_counter
             + self._dp_rank * 0xD1B54A32D192ED03) & (2 ** 64 - 1)
        x ^= x >> 31
        x = (x * 0x94D049BB133111EB) & (2 ** 64 - 1)
        return int(x ^ (x >> 29)) & (2 ** 62 - 1)

    def nonfinite_loss_mask(self, sticky=False, clear=False):
        """Device int32 bitmask, bit i set when modality i's loss was NaN / Inf (set by the loss
        kernel): of the last forward with targets, or (sticky=True) of every
        forward since the sticky word was last cleared (clear=True clears it). A copy, no sync."""
        if self._ws is None:
            return None
        off = ML.lib().mmt_loss_flag_offset(self._ctx, self._ws_batch) + (4 if sticky else 0)
        w = self._ws[off:off + 4]
        out = w.view(torch.int32).clone()
        if sticky and self._sticky_carry:
            out |= self._sticky_carry
        if clear:
            w.zero_()
            if sticky:
                self._sticky_carry = 0
        return out

    def backward_stage_ranges(self):
        """[(begin, end)] of the flat gradient finalised by each backward stage, in execution order
        (post block, layers L-1..0, embeddings); see mmt_backward_stage_range in include/mmt.h."""
        L = ML.lib()
        out = []
        b, e = ML.c_i64(), ML.c_i64()
        for s in range(L.mmt_backward_stage_count(self._ctx)):
            ML.check(L.mmt_backward_stage_range(self._ctx, s, ctypes.byref(b), ctypes.byref(e)), self._ctx,
                     "mmt_backward_stage_range")
            out.append((b.value, e.value))
        return out

    def tensor_segments(self):
        """Every reference tensor of the active prefix (the part of the flat buffer that gets gradients), in
        offset order: a dict with `names`, `begins`, `ends` (element offsets into flat_params / its gradient),
        and the segment table of mmt_tensor_stats: `bounds` (the tensors and the gaps between them, see
        mmt_stats.build_segments), `named` (index in the table of each tensor) and `device` (the table as an
        int64 device tensor, made once per device and cached). The tensors are asserted disjoint."""
        import mmt_stats
        dev = self.flat_params.device
        seg = getattr(self, "_segments", None)
        if seg is None:
            rows = []
            for name, off, shp, _ in self._tensors:
                if off >= self._n_active:
                    continue
                n = 1
                for s in shp:
                    n *= s
                rows.append((off, off + n, name))
            rows.sort()
            names, begins, ends = [r[2] for r in rows], [r[0] for r in rows], [r[1] for r in rows]
            bounds, named = mmt_stats.build_segments(names, begins, ends)  # raises when two tensors overlap
            assert not ends or ends[-1] <= self._n_active
            seg = self._segments = {"names": names, "begins": begins, "ends": ends, "bounds": bounds, "named": named,
                                    "device": None}
        if dev.type == "cuda" and (seg["device"] is None or seg["device"].device != dev):
            seg["device"] = torch.tensor(seg["bounds"], dtype=torch.int64).to(dev)
        return seg

    def tensor_stats(self, which="grad"):
        """A one-shot snapshot of the per-tensor statistics of the gradient ("grad") or of the parameters
        ("param"): an mmt_stats.StatsReport (sum of squares, largest magnitude, NaN / Inf counts and the first
        non-finite position per reference tensor, rollups per backward stage). One device pass, one sync."""
        import mmt_stats
        if which not in ("grad", "param"):
            raise ValueError(f"tensor_stats: which must be 'grad' or 'param', got {which!r}")
        buf = self.flat_params.grad if which == "grad" else self.flat_params.detach()
        if buf is None:
            raise RuntimeError("tensor_stats('grad'): flat_params.grad is None (run a backward first)")
        st = getattr(self, "_stats_oneshot", None)
        if st is None or st._rec is None or st._rec.device != buf.device:
            st = self._stats_oneshot = mmt_stats.TensorStats(self, mode="every")
        st.record(buf)
        return st.read(rearm=True)

    def set_grad_accumulation(self, on):
        """In-place gradient accumulation (include/mmt.h, mmt_set_grad_accumulate). When on, the backward
        writes straight into `flat_params.grad` instead of handing autograd a fresh gradient that
        AccumulateGrad adds in another pass: if `.grad` is None the engine overwrites a persistent buffer
        the model owns and that buffer becomes `.grad`; otherwise the engine adds into `.grad` in place.
        `zero_grad(set_to_none=True)` between optimizer steps keeps its meaning (the next backward
        overwrites), `reference_grad_views()` keeps working. Averaging over k micro-batches is the caller's
        loss scale: `(sum(losses) / k).backward()` costs nothing extra, the engine differentiates
        sum_i loss_grads[i] * loss_i anyway.
        In this mode autograd sees no gradient for `flat_params`, so tensor hooks registered on it do not
        fire with a gradient (torch skips them or calls them with None, depending on its version; read
        `flat_params.grad` after the backward instead), and a `.grad` kept from before a `zero_grad(set_to_none=True)` is the model's buffer: the next
        backward overwrites it (clone it to keep it)."""
        self.grad_accumulation = bool(on)

    @contextlib.contextmanager
    def no_sync(self):
        """In the spirit of DistributedDataParallel.no_sync: inside the context a data-parallel model
        (mmt_dist.enable_data_parallel) runs the unstaged backward and exchanges nothing; the first backward
        outside it all-reduces what has accumulated. Needs set_grad_accumulation(True) when data parallel
        (the all-reduce must see the accumulated sums, not the last micro-batch alone). Without data
        parallelism it changes nothing."""
        if self._grad_sync is not None and not self.grad_accumulation:
            raise RuntimeError("no_sync() on a data-parallel model needs set_grad_accumulation(True)")
        old = self._no_sync
        self._no_sync = True
        try:
            yield
        finally:
            self._no_sync = old

    def _grad_target(self, flat):
        """(buffer the engine writes, accumulate?) of the in-place mode."""
        p = self.flat_params
        if p.grad is None:
            b = self._grad_buf
            if b is None or b.device != flat.device or b.numel() != flat.numel():
                b = self._grad_buf = torch.empty_like(flat.detach())
            return b, False
        g = p.grad
        if g.dtype != torch.float32 or g.device != flat.device or not g.is_contiguous() or g.numel() != flat.numel():
            raise RuntimeError("gradient accumulation needs flat_params.grad as a contiguous fp32 tensor on the "
                               "model's device")
        return g, True

    def _launch_backward(self, g_losses):
        L = ML.lib()
        flat = self._last[0]
        g = g_losses.detach().to(dtype=torch.float32).contiguous()
        inplace = self.grad_accumulation
        if inplace:
            grad, acc = self._grad_target(flat)
            ML.check(L.mmt_set_grad_accumulate(self._ctx, 1 if acc else 0), self._ctx, "mmt_set_grad_accumulate")
        else:
            grad = torch.empty_like(flat)
        sync = None if self._no_sync else self._grad_sync
        try:
            grad = self._run_backward(L, flat, g, grad, sync)
        finally:
            if inplace:
                L.mmt_set_grad_accumulate(self._ctx, 0)
        if inplace:
            if self.flat_params.grad is None:
                self.flat_params.grad = grad
            return None  # nothing for AccumulateGrad to add
        return grad

    def _run_backward(self, L, flat, g, grad, sync):
        with torch.cuda.device(flat.device):
            if sync is None:
                rc = L.mmt_backward(self._ctx, ML.stream_ptr(flat.device), ML.ptr(g), ML.ptr(flat), ML.ptr(grad),
                                    ML.ptr(self._ws))
                ML.check(rc, self._ctx, "mmt_backward")
                return grad
            # data parallel (mmt_dist): stage by stage, each finished bucket all-reduced while the
            # next stages compute
            for s in range(L.mmt_backward_stage_count(self._ctx)):
                rc = L.mmt_backward_stage(self._ctx, ML.stream_ptr(flat.device), s, ML.ptr(g), ML.ptr(flat),
                                          ML.ptr(grad), ML.ptr(self._ws))
                ML.check(rc, self._ctx, "mmt_backward_stage")
                sync.stage_done(s, grad)
            sync.finish()
        return grad

    def forward(self, idx_list, targets_list=None):
        """model.py:380-402: returns (logits_list, losses_list | None)."""
        M = self.num_modalities
        if len(idx_list) != M:
            raise ValueError(f"expected {M} index tensors, got {len(idx_list)}")
        flat = self.flat_params
        if flat.device.type != "cuda":
            raise RuntimeError("MultimodalTransformer (libmmt_hip) runs only on a ROCm GPU: call .to('cuda') "
                               "(there is no CPU path)")
        B, T = idx_list[0].shape
        if T > self.block_size:
            raise ValueError(f"sequence length {T} exceeds block_size {self.block_size}")
        if T < self.block_size and targets_list is not None:
            raise NotImplementedError(f"training on sequence length {T} < block_size {self.block_size}: the training "
                                      f"batches of the reference are always block_size long")
        idx = [t.to(device=flat.device, dtype=torch.long).contiguous() for t in idx_list]
        for t in idx:
            if tuple(t.shape) != (B, T):
                raise ValueError("all modalities must share the [B, T] batch shape")
        if T < self.block_size:
            # causal: position t sees tokens <= t only, so right padding leaves positions < T unchanged
            pad = self.block_size - T
            idx = [torch.nn.functional.pad(t, (0, pad)) for t in idx]
            logits = _MmtStep.apply(flat, self, False, M, *idx)
            return [lg[:, :T] for lg in logits], None
        tensors = list(idx)
        if targets_list is not None:
            tensors += [t.to(device=flat.device, dtype=torch.long).contiguous() for t in targets_list]
        training = bool(self.training and self.dropout_p > 0.0)
        outs = _MmtStep.apply(flat, self, training, M, *tensors)
        logits = list(outs[:M])
        if targets_list is None:
            return logits, None
        losses = outs[M]
        return logits, [losses[i] for i in range(M)]

    @torch.no_grad()
    def generate(self, idx_list, max_new_tokens=1, modality_to_generate=0, use_cache=True, sample_fn=None, *,
                 temperature=None, top_k=None, top_p=None, seed=None, return_logprobs=False, logits_hook=None,
                 num_samples=None, given=None, evidence=None, resample_every=1, ess_threshold=0.5, forecast=None,
                 horizon=None, realised=None, rolling=False):
        """model.py:404-446: per new token, the logits of the last position of the (block_size
        cropped) context, a sample from the softmax of the target modality's last logits
        (torch.multinomial, as the reference; `sample_fn(probs) -> [B, 1]` overrides it), appended;
        the other modalities are padded with their last token or cropped to the same length.

        The reference re-runs the whole forward per token. Here, while the sequence still fits the
        block (positions do not shift), the first step is one forward over the prompt (the prefill,
        which leaves the keys / values of every position in the workspace) and every later step is
        ONE position through the KV-cache decode of the engine (mmt_decode_step): the same logits
        (causal attention, absolute positions) at O(t) instead of O(block_size) attention and no
        re-run of the prompt's GEMMs. Once the sequence outgrows the block every position shifts
        and it falls back to the reference's full re-forward. use_cache=False (or training mode
        with dropout, where the reference's forward samples dropout, or the fp8 precision, whose
        forward GEMMs the bf16 decode would not reproduce) always re-runs the forward.

        Any of the keywords temperature / top_k / top_p / seed / return_logprobs / logits_hook selects the
        device path (mmt_rollout.py; the rule of mmt_sample in include/mmt.h): sampling
        on the device with draws keyed by (seed, row, position), no torch generator consumed, and with
        return_logprobs=True the return value (sequences, logprobs fp32 [B, max_new_tokens]). Without them
        the body below runs as before.

        num_samples=S (an integer >= 1; it selects the device path too) returns S continuations of every prompt:
        what generate([p.repeat_interleave(S, 0) for p in prompts], ...) returns, row b*S + s being sample s of
        prompt b with its draw at position n keyed by (seed, b*S + s, n), but from ONE prefill over the B prompts
        and decode steps over B*S rows that share each prompt's keys / values (mmt_decode_fanout_step). That engine runs with use_cache, in eval mode or without dropout, at bf16, for
        prompts of one length n0 >= 1 with n0 + max_new_tokens <= block_size; otherwise the prompts are tiled and
        the device path runs as without the keyword. `last_generate_path` says which ran: "fanout" or "tiled".

        rolling=True (with num_samples; pass num_samples=1 for one path) lifts the bound n0 + max_new_tokens <=
        block_size: a forecast from a full context window. Past the block every position shifts, so the tiled call
        re-runs B*S windows of block_size rows per token. But the first p = block_size - j rows of every path's
        window at new token j are the prompt's rows, shifted, and the same for all S paths; only the last m = j are
        the path's own. A rolling step runs one ordinary forward over the B shifted prompts and ONE
        mmt_rolling_step (include/mmt.h) over the B*S*m own rows: B*p + B*S*m rows through the layers where the tiled
        step takes B*S*block_size. While the sequence still fits the block the steps are the fan-out engine's. It runs
        under the fan-out conditions with that bound replaced by n0 <= block_size and max_new_tokens <= block_size;
        `last_generate_path` is "rolling" when the call leaves the block (n0 + max_new_tokens - 1 > block_size),
        "fanout" when it stays inside (bit for bit the call without the keyword), and the call falls back to "tiled"
        otherwise. The logits are those of the tiled re-forward up to rounding, not bit for bit; draws stay keyed by
        (seed, row, position). Both forms, given=, forecast=, horizon=, realised= and evidence="weights" run
        unchanged on rolling steps; evidence="resample" still needs the call to stay inside the block.

        Joint rollouts: modality_to_generate as a sequence of distinct ints (even of one) or "all" samples each of
        those modalities per step from its own head and feeds them back together (always the
        device path: one decode step and one mmt_sample_multi per token). The draw of modality i, row r, position n
        is mmt_sample's with the seed mmt_sample.modality_seed(seed, i), whatever else is generated. given={i:
        int64 [B, N] or [B * S, N]} makes modality i follow the caller's tokens (a scenario, or a series known in
        advance; [B, N] is shared by a prompt's samples); every other modality is held at its last prompt token. In
        this form temperature / top_k / top_p are scalars or {modality: value} dicts, logits_hook(n, logits_list)
        sees the [rows, V_i] views of all modalities, return_logprobs gives (sequences, {i: fp32 [rows, N]}),
        sample_fn and prompts of unequal lengths are refused (plan_joint lists every refusal), and num_samples runs
        the fan-out engine under the conditions above. An int runs exactly as it always did.

        Evidence of a given series (list form with given=): a forced series makes the paths samples of "the model
        with modality i overwritten", not of "the model given that modality i does this". The heads are
        conditionally independent given the history, so the probability of the forced token under its own head is
        the path's importance weight. evidence="weights" scores every given token on the device (one
        mmt_score_multi launch per token over the views the sampler reads, on every path: cached, fan-out, tiled,
        re-forward, fp8) and returns a last element `ev`, a dict: "given_logprobs" {i: fp32 [rows, N]},
        "log_weights" fp64 [rows] (the sum over j, then over the given i ascending), "log_evidence" fp64 [B] (the log
        of the mean weight of a prompt's paths, the estimate of log p(given series | prompt); B = rows without
        num_samples), "ancestors" int32 [points, rows], "resampled" int32 [points, B] and "steps" (the j of every
        resampling point; none here). Sequences and sampled log-probabilities are bit-identical to the call without
        evidence. evidence="resample" also turns the weighted paths into posterior paths (a particle filter,
        mmt_resample in include/mmt.h): after the sampling of new token j, whenever (j + 1) % resample_every == 0 and
        j < N - 1, every prompt whose effective sample size fell below ess_threshold * S redraws its S paths from
        their weights (systematic resampling; the others keep theirs), the sequences, log-probabilities and fan-out
        tails follow their ancestors (mmt_fanout_gather), the weights restart at 1 and log_evidence keeps the
        product. The host follows the fixed schedule and never reads the device's verdict; draws stay keyed by
        (seed, current row, position), so copies of one ancestor diverge at the next step. It needs num_samples
        (at most 4096) and the fan-out engine's conditions and raises ValueError otherwise (no fallback), and it
        holds two fan buffers. Returned rows are the final paths: "given_logprobs" are those of each path's own
        history, "log_weights" the weights since the last resampling point.

        Forecast distributions (list form only; an int is refused, pass [g]): forecast=True, or a dict {"quantiles":
        levels in (0, 1), at most 16 (default 0.05, 0.5, 0.95), "values": {i: fp64 [V_i], non-decreasing in token
        order}, "is_percent": {i: bool}}, adds a last element `fc` = {i: {...}} per generated modality i: per new
        token j and prompt the mixture of the laws the prompt's paths draw token j from (temperature / top-k / top-p
        as the sampler applies them), weighted by the evidence where evidence= is on (mmt_forecast_multi in
        include/mmt.h, one call per token after the sampling, on every path of the list form; with evidence the weights
        are the carried log-weights times the given columns since the last resampling point through j, so step j
        estimates p(token j | prompt, given series through j), taken before a resampling at j). Without
        num_samples every row is a prompt of one path and the pmf is the sampler's own distribution of that row.
        Keys: "pmf" fp32 [Bp, N, V_i]; "ess" fp64 and "live" int32 [Bp, N] (the effective number and the number of
        paths behind each pmf); after the loop one mmt_pmf_stats gives "entropy" (nats), "mean", "var" (of the value;
        NaN without values), "p_down" / "p_flat" / "p_up" (the mass of tokens below / at / above zero for a percent
        series, the prompt's last token of that modality for a value series: at step 0 the reference's directional
        certainty), fp64 [Bp, N]; "quantile_tokens" int32 [Bp, N, Q] and "quantile_values" fp64 [Bp, N, Q] (NaN
        without values). Sequences, log-probabilities and `ev` are bit-identical to the call without forecast=. The
        direction against each path's own previous token at steps j > 0 depends on the path, not on the mixture:
        horizon= reports it. Out of scope: smoothing weights from the whole given series (step j sees the series
        through j only).

        Horizon forecasts (list form only; an int is refused, pass [g]): forecast= gives the law of the token at
        step j, for a percent series the law of ONE step's change. horizon=True, or a dict {"quantiles": levels,
        "values": {i: ...}, "is_percent": {i: bool}, "barriers": {i: at most 8 finite non-zero numbers}} (values and
        is_percent default to forecast='s, when that is given too), adds a last element `hz` = {i: {...}} after
        `fc`, for every generated modality i with values (none: ValueError, a horizon has no meaning on token
        indices): where the series stands after j steps on each path, x_j = ((prod over the steps of 1 + v / 100)
        - 1) * 100 for a percent series and v[token j] - v[the prompt's last token] for a value series, summarised
        over a prompt's paths under their final weights. One mmt_horizon_stats call (include/mmt.h) after the loop,
        over the sequence buffers and, with evidence=, the final log_weights; no torch op or sync per token, on every
        path of the list form (fan-out, tiled, no num_samples: then every row is a prompt of one path). Keys, fp64
        [Bp, N]: "mean", "var" (of x); "p_down" / "p_flat" / "p_up" (the mass of x < 0, == 0, > 0: direction over the
        horizon); "step_down" / "step_flat" / "step_up" (the direction of step j against each path's own previous
        token, the reference's _get_direction_sign); "mean_high" / "mean_low" (the running extremes since the origin,
        which counts as 0); "min" / "max"; "quantile_values" fp64 and "quantile_paths" int32 [Bp, N, Q] (the weighted
        quantile of x and the path s of the prompt that carries it); "hit" fp64 [Bp, N, nb] (the probability of having
        touched barrier u by step j: running high >= u for u > 0, running low <= u for u < 0; it does not decrease in
        j); "ess" fp64 and "live" int32 [Bp]. Under evidence="resample" the rows are the final paths and follow their
        ancestors, so every step's statistic is that of the surviving histories under the final weights: the
        SMOOTHED estimate (given the whole series), not the filtered one forecast= reports; after heavy resampling
        the early steps rest on few distinct ancestors. num_samples > 4096 is refused before the prefill. Sequences,
        log-probabilities, `ev` and `fc` are bit-identical to the call without horizon=.

        Joint horizon forecasts: two more keys of horizon=, "baskets": [{"weights": {i: a_i}, "barriers": [...]}, ...]
        (at most 8; i a generated modality with values, a modality that is not named has coefficient 0) and "pairs":
        "all" or [(i, k), ...] (at most 28), add `hz["joint"]` = {"ess", "live", "modalities", "baskets": [dict per
        basket], "pairs": {(i, k): dict}}: one mmt_horizon_joint call (include/mmt.h) after the mmt_horizon_stats
        call, on the same buffers, origins and log_weights, over the modalities a basket or a pair names. A basket
        dict: "stats" fp64 [Bp, N, 9] and its columns "mean", "var", "p_down", "p_flat", "p_up", "mean_high",
        "mean_low", "min", "max" of y_j = sum_i a_i x_j^(i); "quantile_values", "quantile_rows" and "tail_means" (the
        mean of y below each quantile: the expected shortfall; mirror the weights for the upper tail) [Bp, N, Q];
        "hit" [Bp, N, nb]. A pair dict: "cov", "corr" (NaN where a variance is 0), "var_p", "var_q" fp64 [Bp, N],
        "sign_table" and "step_table" fp64 [Bp, N, 3, 3], the mass of (sign x_i, sign x_k) and of the two step
        directions at [s_i + 1, s_k + 1]. A path that is dead in one of those series is dead for every basket and
        pair. Without the two keys nothing is launched, "joint" is absent and every output is as before; with them
        everything else the call returns is bit-identical. realised= does not score baskets.

        Scored horizons (list form only, needs horizon=): realised={i: int64 [B, N]}, i a generated modality with
        values, is the series that followed each prompt (a backtest: the prompt is the head of a known window, the
        realised row its tail). One mmt_horizon_score call (include/mmt.h) follows the mmt_horizon_stats call, on the
        same buffers, weights, levels and barriers, the origin of both the column before the new ones, and adds a last
        element `sc` = {i: {...}} after `hz`. Keys, fp64 [Bp, N]: "realised" (the realised cumulative change x*),
        "crps" (of the weighted paths at x*), "pit" (mid-PIT), "mean_error" (hz mean - x*), "p_realised_sign" and
        "p_realised_step" (the mass hz gave the sign of x* and the direction of the realised step), "realised_high" /
        "realised_low"; "pinball" fp64 [Bp, N, Q] (of hz's quantile_values) and "brier" fp64 [Bp, N, nb] (of hz's hit);
        and the per-step tables "agg" [N, 10], "aggq" [N, Q, 2], "aggb" [N, nb, 3], "pit_hist" [N, 10] that
        mmt_eval.RolloutMetrics accumulates over calls. A prompt whose realised row holds a token outside the
        vocabulary, or that has no live path, has NaN scores and enters no table. Refused (ValueError) without
        horizon=, in the int form, for a key that is not a generated modality with values and for a tensor that is
        not int64 [B, N]. Sequences, log-probabilities, `ev`, `fc` and `hz` are bit-identical to the call without
        realised=.

        temperature="calibrated" stands for the temperatures set_calibrated_temperatures holds (estimate_loss with
        eval_temperature: fit stores the val fit): the stored number in the int form, {modality: tau} over the
        generated modalities in the list form, resolved before anything else, so the call IS the call with those
        numbers, bit for bit on every engine. ValueError names the first generated modality without one."""
        if isinstance(temperature, str):
            temperature = MR.resolve_calibrated(temperature, self.calibrated_temperatures, modality_to_generate,
                                                self.num_modalities)
        if num_samples is not None:
            num_samples = check_num_samples(num_samples)
        elif rolling:
            raise ValueError("generate: rolling=True rolls the num_samples paths of each prompt: pass num_samples "
                             "(num_samples=1 for one path)")
        plan = plan_joint(modality_to_generate, given, self.vocab_sizes, [tuple(s.shape) for s in idx_list],
                          max_new_tokens, num_samples, evidence, resample_every, ess_threshold, forecast, horizon,
                          realised)
        if plan is not None:
            if sample_fn is not None:
                raise ValueError("generate: sample_fn cannot be combined with a joint rollout (a list of modalities "
                                 "or \"all\"): it samples on the GPU")
            return MR.rollout(self, idx_list, plan, use_cache, temperature, top_k, top_p, seed, return_logprobs,
                              logits_hook, num_samples, rolling=rolling)
        if not (temperature is None and top_k is None and top_p is None and seed is None and not return_logprobs
                and logits_hook is None and num_samples is None):
            if sample_fn is not None:
                raise ValueError("generate: sample_fn cannot be combined with temperature / top_k / top_p / seed / "
                                 "return_logprobs / logits_hook / num_samples (the device path samples on the GPU)")
            return MR.rollout_int(self, idx_list, max_new_tokens, modality_to_generate, use_cache, temperature, top_k,
                                  top_p, seed, return_logprobs, logits_hook, num_samples, rolling)
        sample = sample_fn or (lambda probs: torch.multinomial(probs, num_samples=1))
        return MR.reference_loop(self, [idx.clone() for idx in idx_list], max_new_tokens, modality_to_generate,
                                 use_cache, lambda j, n, last: sample(torch.softmax(last, dim=-1)))

    @torch.no_grad()
    def _decode_step(self, tokens, pos):
        """Logits [B, V_i] of every modality at position `pos` (1 <= pos < block_size), given the
        tokens [B] of that position; the workspace must hold positions < pos (a forward over them,
        then decode steps; include/mmt.h mmt_decode_step)."""
        flat = self.flat_params
        dev = flat.device
        B = tokens[0].shape[0]
        if self._ws is None or self._ws_batch != B:
            raise RuntimeError("_decode_step: no prefill forward at this batch size")
        idx = [t.to(device=dev, dtype=torch.long).contiguous() for t in tokens]
        logits = [torch.empty(B, V, dtype=torch.float32, device=dev) for V in self.vocab_sizes]
        L = ML.lib()
        with torch.cuda.device(dev):
            rc = L.mmt_decode_step(self._ctx, ML.stream_ptr(dev), B, int(pos), ML.ptr_array(idx), ML.ptr(flat),
                                   ML.ptr_array(logits), ML.ptr(self._ws))
        ML.check(rc, self._ctx, "mmt_decode_step")
        self._gen += 1
        self._keep_decode = idx  # alive until the step's kernels have read them
        return logits

    @torch.no_grad()
    def _decode_fanout_step(self, tokens, pos, samples, n0, max_new):
        """Logits [B*S, V_i] of every modality at position `pos` of the B*S sample rows (row b*S + s), given their
        tokens [B*S]; the workspace must hold a prefill of the B prompts (positions < n0), and the steps run
        n0, n0 + 1, ... in order (include/mmt.h mmt_decode_fanout_step). The fan buffer is kept on the model from
        the step at n0 on."""
        flat = self.flat_params
        dev = flat.device
        R = tokens[0].shape[0]
        B = R // samples
        if self._ws is None or self._ws_batch != B or B * samples != R:
            raise RuntimeError("_decode_fanout_step: no prefill forward at this batch size")
        L = ML.lib()
        nbytes = L.mmt_fanout_bytes(self._ctx, B, samples, max_new)
        if nbytes < 0:
            raise ValueError("_decode_fanout_step: batch, samples or max_new out of range")
        if pos == n0 or self._fan is None or self._fan.numel() != nbytes or self._fan.device != dev:
            self._fan = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        idx = [t.to(device=dev, dtype=torch.long).contiguous() for t in tokens]
        logits = [torch.empty(R, V, dtype=torch.float32, device=dev) for V in self.vocab_sizes]
        with torch.cuda.device(dev):
            rc = L.mmt_decode_fanout_step(self._ctx, ML.stream_ptr(dev), B, samples, n0, max_new, int(pos),
                                          ML.ptr_array(idx), ML.ptr(flat), ML.ptr_array(logits), ML.ptr(self._ws),
                                          ML.ptr(self._fan))
        ML.check(rc, self._ctx, "mmt_decode_fanout_step")
        self._keep_decode = idx  # alive until the step's kernels have read them
        return logits

    @torch.no_grad()
    def _rolling_step(self, seqs, samples, p, m):
        """Logits [B*S, V_i] of every modality at position p + m - 1 of the B*S paths (row b*S + s), given the int64
        [B*S, cap >= p + m] sequences `seqs` whose columns p..p+m-1 are the paths' own tokens; the workspace must
        hold a forward over the B prompts' first p positions (include/mmt.h mmt_rolling_step)."""
        flat = self.flat_params
        dev = flat.device
        R, cap = seqs[0].shape
        B = R // samples
        if self._ws is None or self._ws_batch != B or B * samples != R:
            raise RuntimeError("_rolling_step: no forward at this batch size")
        L = ML.lib()
        nbytes = L.mmt_rolling_bytes(self._ctx, B, samples, m)
        if nbytes < 0:
            raise ValueError("_rolling_step: batch, samples or m out of range")
        roll = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        idx = [t.to(device=dev, dtype=torch.long).contiguous() for t in seqs]
        tail = ML.ptr_array(idx)
        for i, t in enumerate(idx):
            tail[i] = t.data_ptr() + 8 * p
        logits = [torch.empty(R, V, dtype=torch.float32, device=dev) for V in self.vocab_sizes]
        with torch.cuda.device(dev):
            rc = L.mmt_rolling_step(self._ctx, ML.stream_ptr(dev), B, samples, int(p), int(m), tail, cap, ML.ptr(flat),
                                    ML.ptr_array(logits), ML.ptr(self._ws), ML.ptr(roll))
        ML.check(rc, self._ctx, "mmt_rolling_step")
        self._keep_decode = idx + [roll]  # alive until the step's kernels have read them
        return logits

    def __del__(self):
        try:
            if getattr(self, "_ctx", None):
                ML.lib().mmt_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass
