"""The attention launch plan (csrc/mmt_attn_plan.h) read through mmt_op_attention_plan: host arithmetic, no device.
Shared by tests/test_attn_plan_cpu.py, which pins the policy, and by the GPU tests whose rows are named after the
kernels they are meant to reach; the tables of those rows live here so that both see the same ones."""
import ctypes

FWD, BWD, MASK = 0, 1, 2
FAMILY = ["chunk_fwd", "chunk_dq", "chunk_dkdv", "ring64_fwd", "ring64_dq", "ring64_dkdv", "onepass64", "onepass32",
          "oc32_fwd", "mask"]
LD = ["q_ld", "kv_ld", "kv_hs", "o_ld", "dout_ld", "dq_ld", "dkv_ld", "dkv_hs", "dq32_ld", "h1_ld"]
Q2, OC, SCRATCH, DET = 0x100, 0x200, 0x400, 0x800              # fields present
Q_8MOD16, DO_8MOD16, DQ_8MOD16, O_8MOD16 = 0x1000, 0x2000, 0x4000, 0x8000
ASSUME_Q2 = 0x10000
PLAN_INTS = 32


def call(pas, B, T, H, hs, ns=1, drop=False, flags=0, **ld):
    """ns: streams of the one problem, or a list with one entry per problem; drop: all problems, or a list."""
    ns = [ns] if isinstance(ns, int) else list(ns)
    drop = [bool(drop)] * len(ns) if isinstance(drop, (bool, int)) else list(drop)
    assert set(ld) <= set(LD) and len(drop) == len(ns)
    return dict(pas=pas, B=B, T=T, H=H, hs=hs, ns=ns, ld=[ld.get(k, 0) for k in LD],
                flags=flags | sum(1 << g for g, d in enumerate(drop) if d))


def raw_plan(L, c):
    n = len(c["ns"])
    out = (ctypes.c_int32 * PLAN_INTS)()
    rc = L.mmt_op_attention_plan(c["pas"], n, c["B"], c["T"], c["H"], c["hs"], (ctypes.c_int32 * max(n, 1))(*c["ns"]),
                                 (ctypes.c_int32 * 10)(*c["ld"]), c["flags"], out)
    assert rc == 0, rc
    return list(out)


def readable(p):
    """"invalid", "empty", or one (family, template arguments as the kernel's name has them, grid) per launch."""
    status, n = p[0], p[1]
    if status:
        return ["ok", "empty", "invalid"][status]
    out = []
    for i in range(n):
        fam, hs, drop, ms, q2, det, oc, occ, depth, g, gx, gy, gz, wg = p[2 + 14 * i: 16 + 14 * i]
        assert wg == 256
        name = FAMILY[fam]
        args = {"chunk": (hs, drop), "ring64_dkdv": (drop, occ, depth, 4), "onepass32": (drop, ms, q2, det, oc),
                "oc32_fwd": (drop,), "mask": (g,)}.get("chunk" if name.startswith("chunk") else name, (drop, depth))
        out.append((name, args, (gx, gy, gz)))
    return tuple(out)


def plan(L, c):
    return readable(raw_plan(L, c))


def families(L, c):
    p = plan(L, c)
    return p if isinstance(p, str) else tuple(l[0] for l in p)


# ------------------------------------------------------------------ the GPU tests' tables and what their names claim
# tests/test_gpu_attn_dropout.py::test_readout: (path, mmt_attn_set_ring, hs, T, streams, fp32 dQ scratch); B 2, H 3
PATHS = [
    ("chunked", 15, 16, 45, 1, False), ("chunked", 15, 16, 45, 2, False),
    ("chunked", 15, 32, 37, 1, False), ("chunked", 15, 32, 37, 3, False),
    ("chunked", 15, 32, 300, 1, False), ("chunked", 15, 32, 300, 3, False),  # past the 256-row chunk
    ("chunked", 15, 48, 96, 2, False),
    ("onepass32", 79, 32, 37, 1, False), ("onepass32", 79, 32, 256, 1, False),
    ("onepass32-scratch", 79 | 128, 32, 100, 3, True),
    ("chunked64", 0, 64, 33, 1, False), ("chunked64", 0, 64, 33, 2, False),
    ("chunked64", 0, 64, 160, 1, False), ("chunked64", 0, 64, 160, 2, False),  # past the 128-row chunk
    ("ring64", 15, 64, 160, 1, False), ("ring64", 15, 64, 160, 3, False),
    ("ring64", 15, 64, 300, 1, False), ("ring64", 15, 64, 300, 3, False),
    ("onepass64", 47, 64, 300, 1, False),
]
# a path's name -> (forward family, backward families)
PATH_FAMILIES = {
    "chunked": ("chunk_fwd", ("chunk_dq", "chunk_dkdv")),
    "onepass32": ("chunk_fwd", ("onepass32",)),
    "onepass32-scratch": ("chunk_fwd", ("onepass32",)),
    "chunked64": ("chunk_fwd", ("chunk_dq", "chunk_dkdv")),
    "ring64": ("ring64_fwd", ("ring64_dq", "ring64_dkdv")),
    "onepass64": ("ring64_fwd", ("onepass64",)),
}
# tests/test_gpu_kernels.py::test_attention_fwd_bwd_dropout: one T per path above (the larger):
# (ring, hs, T, streams, scratch); B 2, H 3
DROP_PATHS = [(15, 16, 45, 1, False), (15, 16, 45, 2, False), (15, 32, 300, 1, False), (15, 32, 300, 3, False),
              (15, 48, 96, 2, False), (79, 32, 256, 1, False), (79 | 128, 32, 100, 3, True), (0, 64, 160, 1, False),
              (0, 64, 160, 2, False), (15, 64, 300, 1, False), (15, 64, 300, 3, False), (47, 64, 300, 1, False)]
# tests/test_gpu_kernels.py::test_attention_hs64_backward_variants: rings x (B, T, H, streams)
HS64_RINGS = [0, 1, 3, 7, 8, 15, 47]
HS64_SHAPES = [(2, 100, 2, 1), (1, 520, 2, 2), (1, 1024, 1, 1), (2, 300, 2, 3), (1, 33, 2, 1), (3, 64, 2, 7),
               (2, 512, 2, 1), (1, 500, 3, 1), (3, 7, 2, 1), (1, 96, 1, 1)]
# what that test's docstring says of each knob value: (forward, dQ pass, dK/dV pass, its waves per SIMD); 47 is 15
# with the one-pass backward where T <= 512 and there is one KV stream
HS64_VARIANT = {0: ("chunk_fwd", "chunk_dq", "chunk_dkdv", 0), 1: ("chunk_fwd", "chunk_dq", "ring64_dkdv", 2),
                3: ("chunk_fwd", "ring64_dq", "ring64_dkdv", 2), 7: ("chunk_fwd", "ring64_dq", "ring64_dkdv", 3),
                8: ("ring64_fwd", "chunk_dq", "chunk_dkdv", 0), 15: ("ring64_fwd", "ring64_dq", "ring64_dkdv", 3),
                47: ("ring64_fwd", "ring64_dq", "ring64_dkdv", 3)}
# tests/test_gpu_kernels.py::test_attention_hs32_backward_variants: rings x (B, T, H, streams, scratch)
HS32_RINGS = [79 | 128, 79, 15]
HS32_SHAPES = [(2, 256, 8, 1, False), (3, 37, 2, 1, False), (1, 2, 2, 1, False), (2, 255, 1, 1, False),
               (1, 33, 4, 1, False), (4, 224, 2, 1, False), (2, 256, 2, 2, False), (1, 300, 2, 1, False),
               (2, 256, 2, 3, True), (3, 37, 2, 2, True), (1, 100, 4, 7, True), (2, 64, 1, 4, True), (1, 300, 2, 3, True)]


def hs64_claim(ring, T, ns):
    """(forward families, backward families, dK/dV ring waves per SIMD or 0) of a hs-64 variant row."""
    fwd, dq, dkdv, occ = HS64_VARIANT[ring]
    if ring == 47 and T <= 512 and ns == 1:
        return (fwd,), ("onepass64",), 0
    return (fwd,), (dq, dkdv), occ


def hs32_claim(ring, T, ns, scratch):
    """Backward families of a hs-32 variant row: the one-pass kernel under bit 6 at T <= 256, for several KV streams
    only under bit 7 with scratch; "without scratch the multi-stream cases, and every T > 256 case, take the two-pass
    pair under either knob"."""
    one = bool(ring & 64) and T <= 256 and (ns == 1 or (bool(ring & 128) and scratch))
    return ("onepass32",) if one else ("chunk_dq", "chunk_dkdv")


def kernel_test_call(pas, B, T, H, hs, ns, scratch=False, drop=False):
    """The launch tests/test_gpu_kernels.py::test_attention_fwd_bwd makes: the engine's interleaved [R, 3C] rows with
    one stream, q [R, C] and per-stream [R, 2C] rows of per-head [K | V] with several."""
    C = H * hs
    ld = (dict(q_ld=3 * C, kv_ld=3 * C, dq_ld=3 * C, dkv_ld=3 * C) if ns == 1 else
          dict(kv_ld=2 * C, kv_hs=2 * hs, dkv_ld=2 * C, dkv_hs=2 * hs))
    if scratch:
        ld["dq32_ld"] = C + 4
    return call(pas, B, T, H, hs, ns, drop, SCRATCH if scratch else 0, **ld)


def readout_call(pas, T, hs, ns, scratch):
    """The launch tests/test_gpu_attn_dropout.py::_Problem makes (B 2, H 3, dropout on, 8 pad columns per output row)."""
    C = 3 * hs
    ld = dict(o_ld=C + 8, dq_ld=C + 8, dkv_ld=C + 8)
    if scratch:
        ld["dq32_ld"] = C + 4
    return call(pas, 2, T, 3, hs, ns, True, SCRATCH if scratch else 0, **ld)
