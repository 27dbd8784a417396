"""The recorded rows of tests/test_attn_plan_cpu.py: which kernels the op entries launch, read from a kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/attn_plan_trace.py --record DIR/cases.json
    VAR=val rocprofv3 ... -- python tools/attn_plan_trace.py --record DIR/cases.json --env VAR=val
    python tools/attn_plan_trace.py --decode DIR DIR/cases.json DIR/plans.json
    python tools/attn_plan_trace.py --merge OUT.json PLANS.json [PLANS.json ...]

--record makes one launch per "rec" row of the test's CASES through mmt_op_attention_fwd_drop / _bwd_drop,
mmt_op_attention_fwd_h1_drop / _bwd_h1_drop and mmt_op_attention_mask on zeroed buffers, under the row's setter values,
in the library MMT_LIB_PATH names (default: this tree's; e.g. a build of the commit before the plan function), with a
one-block colsum launch between cases, and writes [case, status] per call. Without --env: the rows that set no
variable; with it: the rows of that variable's value, which the caller sets for the process. --decode reads the trace
beside it into {case: plan} in the form of tests/attn_plan.readable ("invalid" / "empty" when nothing was launched and
the call returned an error / success). --merge joins such files into one fixture (tests/golden/attn_plan_rec.json),
one case per line. Nothing but the kernel trace is collected; no counters.
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "trade-aid-multimodal-transformer_amd"), os.path.join(REPO, "tests")]

def _load():
    global torch, ML, AP, TC, L
    import torch
    import attn_plan as AP
    import mmt_lib as ML
    import test_attn_plan_cpu as TC
    L = ML.lib()


DEV = "cuda"
S = lambda: ML.stream_ptr(DEV)
MAXS = 8


def z(n, dtype):
    return torch.zeros(int(n) + 256, dtype=dtype, device=DEV)


def arr(ts):
    return (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])


def separator(sep):
    rc = L.mmt_op_colsum(S(), 1, 1, ML.ptr(sep[0]), 8, ML.ptr(sep[1]), 1.0)
    assert rc == 0, rc


def run(c):
    pas, B, T, H, hs, nsl, ldv, flags = c["pas"], c["B"], c["T"], c["H"], c["hs"], c["ns"], c["ld"], c["flags"]
    bf, f32, i32 = torch.bfloat16, torch.float32, torch.int32
    nd = L.mmt_op_attention_mask_dwords(B, H, T)
    if pas == AP.MASK:
        n = len(nsl)
        bufs = [[z(nd, i32) for _ in range(ns)] for ns in nsl]
        ptrs = (ctypes.c_void_p * (n * MAXS))()
        for g in range(n):
            for j in range(nsl[g]):
                ptrs[g * MAXS + j] = bufs[g][j].data_ptr()
        thr = [(flags >> g) & 1 for g in range(n)]
        return L.mmt_op_attention_mask(S(), n, B, T, H, (ctypes.c_int32 * n)(*nsl), (ctypes.c_uint32 * n)(*[7] * n),
                                       (ctypes.c_uint32 * n)(*thr), ptrs)
    assert len(nsl) == 1 and not (flags & 0x1F800)
    ns, C, R = nsl[0], H * hs, B * T
    dflt = [C, C, hs, C, C, C, C, hs, C, 3 * H * 16]
    q_ld, kv_ld, kv_hs, o_ld, dout_ld, dq_ld, dkv_ld, dkv_hs, dq32_ld, h1_ld = [v or d for v, d in zip(ldv, dflt)]
    rows = lambda ld: (R + 8) * max(ld, C, kv_hs * H, dkv_hs * H)
    drop = flags & 1
    key, thr, scale = 7, 1 if drop else 0, 1.0
    o, lse = z(rows(o_ld), bf), [z(B * H * T, f32) for _ in range(ns)]
    dm = [z(nd, i32) for _ in range(ns)]
    do = z(rows(dout_ld), bf)
    if flags & AP.OC:
        assert hs == 32 and ns == 1
        h1, w2 = z(rows(h1_ld), bf), z(3 * H * 512, f32)
        if pas == AP.FWD:
            return L.mmt_op_attention_fwd_h1_drop(S(), B, T, H, ML.ptr(h1), h1_ld, ML.ptr(w2), ML.ptr(o), o_ld, ML.ptr(lse[0]),
                                                  key, thr, scale, ML.ptr(dm[0]))
        assert flags & AP.Q2
        dh1, dw2, db1 = z(rows(h1_ld), bf), z(3 * H * 512, f32), z(3 * H * 16, f32)
        return L.mmt_op_attention_bwd_h1_drop(S(), B, T, H, ML.ptr(h1), h1_ld, ML.ptr(w2), ML.ptr(o), o_ld, ML.ptr(lse[0]),
                                              ML.ptr(do), dout_ld, ML.ptr(dh1), ML.ptr(dw2), ML.ptr(db1), key, thr, scale,
                                              ML.ptr(dm[0]))
    assert not (flags & AP.Q2)
    q = z(rows(q_ld), bf)
    k, v = [z(rows(kv_ld), bf) for _ in range(ns)], [z(rows(kv_ld), bf) for _ in range(ns)]
    oj = [z(rows(o_ld), bf) for _ in range(ns)]
    head = (S(), B, T, H, hs, ns, ML.ptr(q), q_ld, arr(k), arr(v), kv_ld, kv_hs, ML.ptr(o), o_ld, arr(oj), arr(lse))
    if pas == AP.FWD:
        return L.mmt_op_attention_fwd_drop(*head, key, thr, scale, arr(dm))
    dvec = [z(B * H * T, f32) for _ in range(ns)]
    dq = z(rows(dq_ld), bf)
    dk, dv = [z(rows(dkv_ld), bf) for _ in range(ns)], [z(rows(dkv_ld), bf) for _ in range(ns)]
    dq32 = z((R + 8) * max(dq32_ld, C), f32) if flags & AP.SCRATCH else None
    return L.mmt_op_attention_bwd_drop(*head, ML.ptr(do), dout_ld, arr(dvec), ML.ptr(dq), dq_ld, arr(dk), arr(dv), dkv_ld,
                                       dkv_hs, ML.ptr(dq32), dq32_ld if dq32 is not None else 0, key, thr, scale, arr(dm))


def record(log, envkey):
    sep = (torch.zeros(64, dtype=torch.bfloat16, device=DEV), torch.zeros(64, device=DEV))
    out = []
    for name, row in TC.CASES.items():
        if row[0] != "rec":
            continue
        knob = row[1]
        env = knob.get("env")
        if (env is None) != (envkey is None) or (env and "%s=%s" % next(iter(env.items())) != envkey):
            continue
        if env:
            assert all(os.environ.get(k) == v for k, v in env.items())
        if not env:
            old = L.mmt_attn_set_ring(knob.get("ring", TC.DEFAULT_RING))
        g_old = L.mmt_attn_set_mask_g(knob.get("mask_g", 0))
        separator(sep)
        rc = run(row[2])
        torch.cuda.synchronize()
        if not env:
            L.mmt_attn_set_ring(old)
        L.mmt_attn_set_mask_g(g_old)
        out.append([name, rc])
    separator(sep)
    torch.cuda.synchronize()
    json.dump(out, open(log, "w"))
    print(f"[attn_plan_trace] {len(out)} cases -> {log}")




NAMES = {"attn_fwd_kernel": "chunk_fwd", "attn_bwd_dq_kernel": "chunk_dq", "attn_bwd_dkdv1_kernel": "chunk_dkdv",
         "attn_fwd_ring64x2": "ring64_fwd", "attn_bwd_dq_ring64x2": "ring64_dq", "attn_bwd_dkdv_ring64": "ring64_dkdv",
         "attn_bwd_fused64": "onepass64", "attn_bwd_fused32": "onepass32", "attn_fwd_oc32_kernel": "oc32_fwd",
         "attn_mask_kernel": "mask"}


def decode(d, log, out):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    key = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))
    seq = []
    for r in rows:
        n = r["Kernel_Name"]
        if "colsum_kernel" in n:
            seq.append(None)
            continue
        m = re.search(r"(attn_\w+)<([^>]*)>", n)
        if not m:
            continue
        assert m.group(1) in NAMES, n
        args = [{"true": 1, "false": 0}.get(a.strip(), a.strip()) for a in m.group(2).split(",")]
        args = [int(a) for a in args]
        wg = [int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"]
        grid = [int(r[f"Grid_Size_{a}"]) for a in "XYZ"]
        assert wg == [256, 1, 1], (n, wg)
        assert grid[0] % 256 == 0
        seq.append([NAMES[m.group(1)], args, [grid[0] // 256, grid[1], grid[2]]])
    cases = json.load(open(log))
    assert seq[0] is None and seq[-1] is None and seq.count(None) == len(cases) + 1, (seq.count(None), len(cases))
    plans, i = {}, 1
    for name, rc in cases:
        ks = []
        while seq[i] is not None:
            ks.append(seq[i])
            i += 1
        i += 1
        assert rc == 0 or not ks, (name, rc, ks)
        plans[name] = ks if ks else ("empty" if rc == 0 else "invalid")
    dump(plans, out)
    print(f"[attn_plan_trace] {len(plans)} cases, {sum(len(v) for v in plans.values() if isinstance(v, list))} launches -> {out}")



def dump(plans, out):
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(plans[k])}" for k in sorted(plans)) + "\n}\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", metavar="LOG")
    ap.add_argument("--env", default=None, metavar="VAR=val")
    ap.add_argument("--decode", nargs=3, metavar=("DIR", "LOG", "OUT"))
    ap.add_argument("--merge", nargs="+", metavar="JSON")
    a = ap.parse_args()
    if a.record:
        _load()
        record(a.record, a.env)
    elif a.decode:
        decode(*a.decode)
    elif a.merge:
        plans = {}
        for f in a.merge[1:]:
            plans.update(json.load(open(f)))
        dump(plans, a.merge[0])
    else:
        ap.error("one of --record, --decode, --merge")
