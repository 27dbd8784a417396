"""Bit identity and launch structure of the host engine (csrc/mmt_engine.hip) between two builds of the tree.

    python tools/engine_identity.py --run OUT                       # this tree: every group, one fresh child each
    python tools/engine_identity.py --run OUT --tree DIR            # the same list in another (built) checkout,
                                                                    # e.g. an export of the parent commit
    python tools/engine_identity.py --compare A B                   # A, B: the two OUT directories (A = the parent)

A group is a fixed list of engine calls on the committed fixtures (tests/golden), seeds pinned; --dump GROUP FILE runs
one group in the tree the script is started from and saves every output as integer bit patterns (NaNs compare).
--run starts this script with `--dump GROUP FILE --tree DIR` once per group (all of them, or --groups a,b), one child
at a time, each under its own time limit, and stops at the first child that fails; the child takes the package, its
built library and the fixtures of DIR. The "probe" group saves, per launch label, the launch count
and the algorithmic flops / bytes (host arithmetic on the descriptors) of one training step; its step is not timed.

Entries named "tol:*" (gradients of the default mode and, in "attn_ops", the stage-2 sums of the one-pass hs-32 attention
backward, whose float atomics add in arrival order) are compared by
rel-L2 against tests/test_gpu_determinism.py's bound, with A's own run-to-run difference printed beside it. Every
other entry must be equal bit for bit.
"""
import argparse
import ctypes
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _use_tree(root):
    """The package (and its built library), the fixtures' loader and the oracle of the checkout at `root`."""
    for p in (os.path.join(root, "trade-aid-multimodal-transformer_amd"), os.path.join(root, "tests"),
              os.path.join(root, "oracle")):
        sys.path.insert(0, p)


GRAD_BOUND = 1e-6  # tests/test_gpu_determinism.py: the same sums in another order
SEED = 0x5EED1234

# every label the engine's launch wrapper can see (a merged weight-gradient launch "a+b" counts under its first part)
LABELS = ["qkv1", "attn_fwd", "proj", "proj0", "proj2", "ffn", "ffn0", "ffn2", "ca_q", "ca_kv", "ca_attn_fwd", "ca_proj",
          "ca_proj0", "ca_proj2", "head0", "head2",
          "head2_dw", "head2_dx", "head0_dw", "head0_dx", "ca_proj2_dw", "ca_proj_dx", "ca_proj2_dx", "ca_proj0_dw",
          "ca_proj0_dx", "ca_attn_bwd", "ca_q_dw", "ca_q_dx", "ca_kv_dw", "ca_kv_dx", "ffn2_dw", "ffn2_dx", "ffn0_dw",
          "ffn0_dx", "proj2_dw", "proj_dx", "proj2_dx", "proj0_dw", "proj0_dx", "attn_bwd", "qkv1_dw", "qkv1_dx",
          "det_sum",
          "dec_qkv1", "dec_proj0", "dec_proj2", "dec_ffn0", "dec_ffn2", "dec_ca_q", "dec_ca_kv", "dec_ca_proj0",
          "dec_ca_proj2", "dec_head0", "dec_head2"]

FWD_BWD = ["f_small", "f_hs32", "f_m1", "f_tiny_v", "f_c1", "f_m8:bf16", "f_m8:fp8"]
ENV_CASES = ["MMT_LN_FUSE=0", "MMT_LN_FUSE_FWD=0", "MMT_LN2_FUSE=0", "MMT_MLP2=0", "MMT_MLP2_BWD=0", "MMT_MLP2_BWD=1",
             "MMT_QKV2_FUSE=0", "MMT_MASK_AHEAD=1", "MMT_MASK_AHEAD=2", "MMT_MASK_T2=0", "MMT_DW_ATTN_SMALL=1",
             "MMT_FLUSH_HOLD=1", "MMT_SIDE_STREAM=0"]
GROUPS = ["eval", "det", "setters", "staged", "decode", "default", "probe", "attn_ops"] + ["env:" + e for e in ENV_CASES]


def _fixture(name):
    from golden_io import model_fixture, scale_fixture
    fx, _, prec = name.partition(":")
    z, meta, cfg, sd, idx, tgt = (scale_fixture if fx in ("f_c1", "f_m8") else model_fixture)(fx)
    return meta, sd, idx, tgt, prec or "bf16"


def _build(name, dropout=0.1, det=False, train=True):
    import torch
    import config_utils
    meta, sd, idx, tgt, prec = _fixture(name)
    config_utils._config_cache = {"n_embd": meta["n_embd"], "n_head": meta["n_head"], "n_layer": meta["n_layer"],
                                  "block_size": meta["block_size"], "dropout": dropout, "device": "cuda",
                                  "batch_size": meta["B"], "eval_iters": 1, "precision": prec}
    import model as mmt_model
    m = mmt_model.MultimodalTransformer(len(meta["V"]), meta["V"],
                                        [[None] * 8 + [c] + [None] * 3 for c in meta["cross"]]).to("cuda")
    full = {k: t for k, t in m.state_dict().items() if k.endswith("tril")}
    full.update(sd)
    m.load_state_dict(full, strict=True)
    m._next_dropout_seed = lambda dev: SEED  # mmt_set_dropout_seed: the same masks in both trees
    m.train(train)
    m.set_deterministic(det)
    return m, meta, [t.cuda() for t in idx], [t.cuda() for t in tgt]


def _fwd_bwd(m, idx, tgt, keep_grad=False):
    import torch
    if not keep_grad:
        m.flat_params.grad = None
    logits, losses = m(idx, tgt)
    sum(losses).backward()
    torch.cuda.synchronize()
    out = {f"logits.{i}": lg.detach() for i, lg in enumerate(logits)}
    out["losses"] = torch.stack([ls.detach() for ls in losses])
    out["grad"] = m.flat_params.grad.detach().clone()
    return out


def _step(name, det=True, **kw):
    m, _, idx, tgt = _build(name, det=det, **kw)
    return _fwd_bwd(m, idx, tgt)


class _NoSync:  # makes model._run_backward take mmt_backward_stage, stage by stage
    def stage_done(self, s, grad):
        pass

    def finish(self):
        pass


def _with(setter, value, fn):
    import mmt_lib as ML
    f = getattr(ML.lib(), setter)
    old = f(value)
    try:
        return fn()
    finally:
        f(old)


# ---------------------------------------------------------------------------------------------- the groups
def group_eval():
    import torch
    out = {}
    for name in ["f_demo"] + FWD_BWD:
        m, _, idx, tgt = _build(name, train=False)
        with torch.no_grad():
            logits, losses = m(idx, tgt)
        torch.cuda.synchronize()
        out[name] = dict({f"logits.{i}": lg for i, lg in enumerate(logits)}, losses=torch.stack(list(losses)))
    return out


def group_det():
    return {name: _step(name) for name in FWD_BWD}


def group_setters():
    import mmt_lib as ML
    out = {}
    for v in (0, 1, 2, 3):
        out[f"f_hs32.onchip{v}"] = _with("mmt_set_attn_qkv_onchip", v, lambda: _step("f_hs32"))
    out["f_hs32.attn_qkv2_0"] = _with("mmt_set_attn_qkv2", 0, lambda: _step("f_hs32"))
    out["f_c1.ffn_fused_0"] = _with("mmt_set_ffn_fused", 0, lambda: _step("f_c1"))
    out["f_c1.relu_bits_1"] = _with("mmt_set_relu_bits", 1, lambda: _step("f_c1"))  # latched by mmt_create
    out["f_c1.drop_copy_fuse_0"] = _with("mmt_set_drop_copy_fuse", 0, lambda: _step("f_c1"))
    m, _, idx, tgt = _build("f_c1", det=True)
    m.set_grad_accumulation(True)
    _fwd_bwd(m, idx, tgt)
    out["f_c1.grad_accumulate"] = _fwd_bwd(m, idx, tgt, keep_grad=True)  # the second micro-batch adds in place
    m, _, idx, tgt = _build("f_c1", det=True)
    ML.check(ML.lib().mmt_set_side_stream(m._ctx, 0), m._ctx, "mmt_set_side_stream")
    out["f_c1.side_stream_0"] = _fwd_bwd(m, idx, tgt)
    return out


def group_staged():
    m, _, idx, tgt = _build("f_small", det=True)
    m._grad_sync = _NoSync()
    return {"f_small.staged": {"grad": _fwd_bwd(m, idx, tgt)["grad"]}}


def group_decode():
    import torch
    import mmt_lib as ML
    L = ML.lib()
    out = {}
    m, meta, _, _ = _build("f_small", train=False)
    T, V = meta["block_size"], meta["V"]
    g = torch.Generator().manual_seed(7)
    draw = lambda rows, *shape: [torch.randint(0, v, (rows,) + shape, generator=g).cuda() for v in V]
    with torch.no_grad():
        for B in (4, 1):
            m(draw(B, T))  # the prefill
            e = out[f"f_small.decode_B{B}"] = {}
            for k, pos in enumerate(range(T - 8, T)):
                for i, lg in enumerate(m._decode_step(draw(B), pos)):
                    e[f"step{k}.logits.{i}"] = lg
        B, S, N = 2, 3, 6
        n0 = T - N
        m(draw(B, T))
        nbytes = L.mmt_fanout_bytes(m._ctx, B, S, N)
        assert nbytes > 0
        fan = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")  # zeroed: the pads no kernel writes compare
        e = out["f_small.fanout"] = {}
        dev = m.flat_params.device
        for k in range(N):
            idx = draw(B * S)
            logits = [torch.empty(B * S, v, dtype=torch.float32, device=dev) for v in V]
            rc = L.mmt_decode_fanout_step(m._ctx, ML.stream_ptr(dev), B, S, n0, N, n0 + k, ML.ptr_array(idx),
                                          ML.ptr(m.flat_params), ML.ptr_array(logits), ML.ptr(m._ws), ML.ptr(fan))
            ML.check(rc, m._ctx, "mmt_decode_fanout_step")
            torch.cuda.synchronize()
            for i, lg in enumerate(logits):
                e[f"step{k}.logits.{i}"] = lg
        e["fan"] = fan.clone()
        fan2 = torch.zeros_like(fan)
        anc = torch.tensor([1, 0, 2, 5, 5, 3], dtype=torch.int32, device=dev)
        rc = L.mmt_fanout_gather(m._ctx, ML.stream_ptr(dev), B, S, n0, N, N, ML.ptr(anc), ML.ptr(fan), ML.ptr(fan2))
        ML.check(rc, m._ctx, "mmt_fanout_gather")
        torch.cuda.synchronize()
        e["fan_gathered"] = fan2
    return out


def group_default():
    """Default mode, dropout on: two runs per fixture; the second run's gradient is A's run-to-run figure."""
    out = {}
    for name in FWD_BWD:
        m, _, idx, tgt = _build(name, det=False)
        a, b = _fwd_bwd(m, idx, tgt), _fwd_bwd(m, idx, tgt)
        a["tol:grad"], a["tol:grad.again"] = a.pop("grad"), b["grad"]
        out[name] = a
    return out


def _attn_op(hs, T, ns, ring, p, scratch=False, B=2, H=2):
    """One forward and one backward through mmt_op_attention_fwd_drop / _bwd_drop under mmt_attn_set_ring(ring)."""
    import torch
    import attn_drop_ref as DR
    import mmt_lib as ML
    L, C, R = ML.lib(), H * hs, B * T
    g = torch.Generator().manual_seed(1000 * hs + 10 * T + ns)
    rnd = lambda: torch.randn(R, C, generator=g).to(torch.bfloat16).cuda()
    z16 = lambda: torch.zeros(R, C, dtype=torch.bfloat16, device="cuda")
    zf = lambda: torch.zeros(B * H * T, device="cuda")
    arr = lambda ts: (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ts])
    q, k, v, do = rnd(), [rnd() for _ in range(ns)], [rnd() for _ in range(ns)], rnd()
    o, oj, lse, dvec = z16(), [z16() for _ in range(ns)], [zf() for _ in range(ns)], [zf() for _ in range(ns)]
    dq, dk, dv = z16(), [z16() for _ in range(ns)], [z16() for _ in range(ns)]
    dq32 = torch.zeros(R, C + 4, device="cuda") if scratch else None
    key, thr, c = (0xA77E0000 + T, DR.thr_of(p), DR.scale_of(p)) if p else (0, 0, 0.0)
    dm = [torch.zeros(L.mmt_op_attention_mask_dwords(B, H, T), dtype=torch.int32, device="cuda") for _ in range(ns)]
    s = ML.stream_ptr("cuda")

    def go():
        if p:
            assert L.mmt_op_attention_mask(s, 1, B, T, H, (ctypes.c_int32 * 1)(ns), (ctypes.c_uint32 * 1)(key),
                                           (ctypes.c_uint32 * 1)(thr), arr(dm)) == 0
        head = (s, B, T, H, hs, ns, ML.ptr(q), C, arr(k), arr(v), C, hs, ML.ptr(o), C, arr(oj), arr(lse))
        assert L.mmt_op_attention_fwd_drop(*head, key, thr, c, arr(dm)) == 0
        assert L.mmt_op_attention_bwd_drop(*head, ML.ptr(do), C, arr(dvec), ML.ptr(dq), C, arr(dk), arr(dv), C, hs,
                                           ML.ptr(dq32), C + 4 if scratch else 0, key, thr, c, arr(dm)) == 0
        torch.cuda.synchronize()
    _with("mmt_attn_set_ring", ring, go)
    out = {"o": o, "dq": dq}
    for j in range(ns):
        out.update({f"oj.{j}": oj[j], f"lse.{j}": lse[j], f"dk.{j}": dk[j], f"dv.{j}": dv[j]})
    return {n: t.float() for n, t in out.items()}


def _attn_h1_op(T, p, B=2, H=2):
    """The same through the on-chip-QKV entries (hs 32): the stage-2 sums dW2 / db1 are float atomics ("tol:")."""
    import torch
    import attn_drop_ref as DR
    import mmt_lib as ML
    L, C, R, ld = ML.lib(), H * 32, B * T, 3 * H * 16
    g = torch.Generator().manual_seed(77 + T)
    h1 = torch.tanh(torch.randn(R, ld, generator=g)).to(torch.bfloat16).cuda()
    w2 = (torch.randn(3 * H, 32, 16, generator=g) * 0.25).cuda()
    do = torch.randn(R, C, generator=g).to(torch.bfloat16).cuda()
    o, lse = torch.zeros(R, C, dtype=torch.bfloat16, device="cuda"), torch.zeros(B * H * T, device="cuda")
    dh1 = torch.zeros(R, ld, dtype=torch.bfloat16, device="cuda")
    key, thr, c = (0xA77E1000 + T, DR.thr_of(p), DR.scale_of(p)) if p else (0, 0, 0.0)
    dm = torch.zeros(L.mmt_op_attention_mask_dwords(B, H, T), dtype=torch.int32, device="cuda")
    s = ML.stream_ptr("cuda")
    if p:
        ptrs = (ctypes.c_void_p * 8)(dm.data_ptr())
        assert L.mmt_op_attention_mask(s, 1, B, T, H, (ctypes.c_int32 * 1)(1), (ctypes.c_uint32 * 1)(key),
                                       (ctypes.c_uint32 * 1)(thr), ptrs) == 0
    assert L.mmt_op_attention_fwd_h1_drop(s, B, T, H, ML.ptr(h1), ld, ML.ptr(w2), ML.ptr(o), C, ML.ptr(lse), key, thr, c,
                                          ML.ptr(dm)) == 0
    sums = []
    for _ in range(2):  # the second run's sums are A's run-to-run figure
        dw2, db1 = torch.zeros(3 * H, 32, 16, device="cuda"), torch.zeros(3 * H * 16, device="cuda")
        assert L.mmt_op_attention_bwd_h1_drop(s, B, T, H, ML.ptr(h1), ld, ML.ptr(w2), ML.ptr(o), C, ML.ptr(lse), ML.ptr(do),
                                              C, ML.ptr(dh1), ML.ptr(dw2), ML.ptr(db1), key, thr, c, ML.ptr(dm)) == 0
        torch.cuda.synchronize()
        sums.append((dw2, db1))
    return {"o": o.float(), "lse": lse, "dh1": dh1.float(), "tol:dw2": sums[0][0], "tol:dw2.again": sums[1][0],
            "tol:db1": sums[0][1], "tol:db1.again": sums[1][1]}


def group_attn_ops():
    """One forward and one backward per attention kernel family through the op entries, without and with dropout."""
    out = {}
    for p in (0.0, 0.1):
        for ring in (0, 15, 47):  # hs 64: chunked, rings, one-pass (one stream)
            for ns in (1, 3):
                out[f"hs64.T160.ns{ns}.ring{ring}.p{p}"] = _attn_op(64, 160, ns, ring, p)
        for T in (37, 256):       # hs 32: one-pass
            out[f"hs32.T{T}.ns1.ring79.p{p}"] = _attn_op(32, T, 1, 79, p)
        out[f"hs32.T100.ns3.ring207.scratch.p{p}"] = _attn_op(32, 100, 3, 79 | 128, p, scratch=True)
        out[f"hs32.T300.ns3.ring79.p{p}"] = _attn_op(32, 300, 3, 79, p)  # the chunked pair at hs 32
        out[f"hs16.T45.ns1.ring79.p{p}"] = _attn_op(16, 45, 1, 79, p)
        out[f"h1.T37.p{p}"] = _attn_h1_op(37, p)
    return out


def group_env(case):
    var, _, val = case.partition("=")
    assert os.environ.get(var) == val, f"{case}: set by --run in the child's environment before the library loads"
    return {f"{name}.{case}": _step(name) for name in ("f_small", "f_c1")}


def probe_step(m, idx, tgt, labels=LABELS, step=None):
    """{label: (launches, flops, bytes)} of one training step (or of `step()`), through mmt_probe_set."""
    import mmt_lib as ML
    L = ML.lib()
    L.mmt_probe_set(m._ctx, ",".join(labels).encode())
    L.mmt_probe_enable(m._ctx, 1)
    try:
        step() if step else _fwd_bwd(m, idx, tgt)
        out = {}
        for i, lab in enumerate(labels):
            ms, n, fl, by = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
            ML.check(L.mmt_probe_read_at(m._ctx, i, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl),
                                         ctypes.byref(by)), m._ctx, "mmt_probe_read_at")
            out[lab] = (n.value, fl.value, by.value)
        return out
    finally:
        L.mmt_probe_set(m._ctx, None)


def group_probe():
    import torch
    out = {}
    for name in ("f_small", "f_hs32", "f_c1", "f_m8:bf16"):
        for det in (True, False):
            m, _, idx, tgt = _build(name, det=det)
            _fwd_bwd(m, idx, tgt)  # (the first step also zeroes the gh1 pads)
            tab = probe_step(m, idx, tgt)
            e = out[f"{name}.{'det' if det else 'default'}"] = {}
            e["launches"] = torch.tensor([tab[k][0] for k in LABELS], dtype=torch.int64)
            e["flops"] = torch.tensor([tab[k][1] for k in LABELS], dtype=torch.float64)
            e["bytes"] = torch.tensor([tab[k][2] for k in LABELS], dtype=torch.float64)
    return out


def dump(group, path):
    import numpy as np
    import torch
    fn = group_env if group.startswith("env:") else globals()["group_" + group]
    calls = fn(group[4:]) if group.startswith("env:") else fn()
    flat = {}
    for call, entries in calls.items():
        for k, t in entries.items():
            t = t.detach().contiguous().cpu()
            bits = {4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()]
            flat[f"{call}/{k}"] = t.view(bits).numpy()
    np.savez(path, **flat)
    print(f"[engine_identity] {group}: {len(calls)} calls, {len(flat)} entries -> {path}")


# ---------------------------------------------------------------------------------------------- driver
def run(out_dir, tree, limit, groups):
    os.makedirs(out_dir, exist_ok=True)
    for group in groups:
        env = {k: v for k, v in os.environ.items() if not k.startswith("MMT_")}
        if group.startswith("env:"):
            var, _, val = group[4:].partition("=")
            env[var] = val
        path = os.path.join(out_dir, group.replace(":", "_").replace("=", "_") + ".npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", group, path, "--tree", os.path.abspath(tree)],
                           env=env, timeout=limit)
        if r.returncode != 0:
            print(f"[engine_identity] {group} failed with status {r.returncode}: stopping")
            return r.returncode
    return 0


def compare(a_dir, b_dir):
    import numpy as np
    files = sorted(f for f in os.listdir(a_dir) if f.endswith(".npz"))
    missing = [f for f in files if not os.path.exists(os.path.join(b_dir, f))]
    bad = len(missing)
    tot_eq = tot = 0
    for f in missing:
        print(f"{f}: missing in {b_dir}")
    for f in files:
        if f in missing:
            continue
        A, B = np.load(os.path.join(a_dir, f)), np.load(os.path.join(b_dir, f))
        if sorted(A.files) != sorted(B.files):
            print(f"{f}: the entry lists differ")
            bad += 1
            continue
        calls = {}
        for k in A.files:
            call, _, entry = k.partition("/")
            eq, n, notes = calls.setdefault(call, [0, 0, []])
            if entry.startswith("tol:"):
                if entry.endswith(".again"):
                    continue
                fa, fb = A[k].view(np.float32).astype(np.float64), B[k].view(np.float32).astype(np.float64)
                again = A[k + ".again"].view(np.float32).astype(np.float64)
                rel = np.linalg.norm(fb - fa) / (np.linalg.norm(fa) + 1e-30)
                own = np.linalg.norm(again - fa) / (np.linalg.norm(fa) + 1e-30)
                same = rel <= GRAD_BOUND
                calls[call][2].append(f"{entry} rel-L2 B vs A {rel:.3e} (A run to run {own:.3e}, bound {GRAD_BOUND:g})")
            else:
                same = A[k].shape == B[k].shape and np.array_equal(A[k], B[k])
                if not same:
                    calls[call][2].append(f"{entry} DIFFERS")
            calls[call][0] += int(same)
            calls[call][1] += 1
        print(f"{f[:-4]}:")
        for call, (eq, n, notes) in sorted(calls.items()):
            print(f"  {call}: {eq}/{n} equal" + "".join("\n      " + s for s in notes))
            tot_eq += eq
            tot += n
        if f.startswith("probe"):
            for k in A.files:
                if k.endswith("/launches"):
                    row = ", ".join(f"{lab} {n}" for lab, n in zip(LABELS, A[k].tolist()) if n)
                    print(f"      {k}: {row}")
    print(f"  TOTAL: {tot} entries compared, {tot_eq} equal")
    print("  RESULT: " + ("all equal" if tot_eq == tot and not bad else "DIFFERENT"))
    return 0 if tot_eq == tot and not bad else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", nargs=2, metavar=("GROUP", "FILE"))
    ap.add_argument("--run", metavar="OUT")
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--groups", default="", help="with --run: a comma-separated subset of the groups")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.dump:
        _use_tree(os.path.abspath(a.tree))
        dump(*a.dump)
    elif a.run:
        groups = a.groups.split(",") if a.groups else GROUPS
        assert all(g in GROUPS for g in groups), groups
        sys.exit(run(a.run, a.tree, a.limit, groups))
    elif a.compare:
        sys.exit(compare(*a.compare))
    else:
        ap.error("one of --dump, --run, --compare")
