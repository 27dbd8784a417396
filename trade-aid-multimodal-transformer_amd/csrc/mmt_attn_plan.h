// The attention launch plan (host only): which kernels an AttnBatch takes, with which template arguments and grids.
// mmt_attn_plan / mmt_attn_mask_plan (mmt_attn.hip) fill one for every launch; the launchers launch what it says, the
// engine and the tests read it. It calls no HIP runtime function and allocates nothing.
#pragma once
#include "mmt_kernels.h"

enum AttnPlanStatus { ATTN_PLAN_OK = 0, ATTN_PLAN_EMPTY /* nothing to launch */, ATTN_PLAN_INVALID };
enum AttnFamily {
  ATTN_CHUNK_FWD = 0,  // attn_fwd_kernel<HS, DROP>                    (mmt_attn.hip)
  ATTN_CHUNK_DQ,       // attn_bwd_dq_kernel<HS, DROP>
  ATTN_CHUNK_DKDV,     // attn_bwd_dkdv1_kernel<HS, DROP>
  ATTN_RING64_FWD,     // attn_fwd_ring64x2<DROP, depth>               (mmt_attn2.hip)
  ATTN_RING64_DQ,      // attn_bwd_dq_ring64x2<DROP, depth>
  ATTN_RING64_DKDV,    // attn_bwd_dkdv_ring64<DROP, occ, depth, 4>
  ATTN_FUSED64,        // attn_bwd_fused64<DROP, depth>
  ATTN_FUSED32,        // attn_bwd_fused32<DROP, MS, Q2, DET, OC>      (mmt_attn.hip)
  ATTN_OC32_FWD,       // attn_fwd_oc32_kernel<DROP>                   (mmt_attn_oc.hip)
  ATTN_MASK            // attn_mask_kernel<g>                          (mmt_attn.hip; mmt_attn_mask_plan only)
};
// mmt_attn_plan's `assume`: the stage-2 eligibility as if every problem carried aligned stage-2 fields (q2_*)
enum { ATTN_ASSUME_Q2 = 1 };

struct AttnLaunch {
  int family, hs;        // AttnFamily; head size (0: the mask kernel)
  int drop;              // DROP: the batch has dropout on
  int ms, q2, det, oc;   // fused32: several KV streams, stage-2 epilogue, deterministic partials, on-chip Q/K/V
  int occ, depth;        // the dK/dV ring's waves per SIMD (2 or 3); ring depth of the mmt_attn2.hip kernels
  int g;                 // the mask kernel's tiles per wave
  int gx, gy, gz, wg;    // grid in workgroups (gz: problems) and workgroup size
};
struct AttnPlan {
  int status;            // AttnPlanStatus; the rest is meaningful when OK
  int nlaunch;           // 1, or 2: the dQ pass, then the dK/dV pass
  AttnLaunch l[2];
  int det_stride[2];     // the deterministic fused32 launch: floats of partials per problem (DetLaunch), a 64-bit
                         // count as its low and high 32 bits (attn_det_stride)
};
inline int64_t attn_det_stride(const AttnPlan& p) {
  return (int64_t)(((uint64_t)(uint32_t)p.det_stride[1] << 32) | (uint32_t)p.det_stride[0]);
}
constexpr int ATTN_PLAN_INTS = sizeof(AttnPlan) / sizeof(int);  // mmt_op_attention_plan writes them in this order

AttnPlan mmt_attn_plan(const AttnBatch& b, int B, int T, int H, int hs, bool bwd, int assume = 0);
AttnPlan mmt_attn_mask_plan(const AttnBatch& b, int B, int T, int H);

// true when mmt_launch_attn_bwd runs this batch on the one-pass hs-32 kernel with one KV stream, which can take the
// Q/K/V stage-2 backward in its epilogue (AttnProblem::q2_*); asked before those fields are set. The plan makes every
// check of the launch first, so a batch the launch would refuse (or one with nothing to launch) answers no. The
// engine's forward also asks it of its forward batch: the backward fields it has not set yet (dQ, dK, dV, their
// leading dimensions) are null / 0 and pass those checks.
inline bool mmt_attn_bwd_fuses_qkv2(const AttnBatch& b, int B, int T, int H, int hs) {
  const AttnPlan p = mmt_attn_plan(b, B, T, H, hs, true, ATTN_ASSUME_Q2);
  return p.status == ATTN_PLAN_OK && p.l[0].family == ATTN_FUSED32 && p.l[0].q2;
}

// Head sizes of the chunked kernels (forward, dQ, dK/dV; each with and without DROP)
#define ATTN_CHUNK_HS(X) X(8) X(16) X(24) X(32) X(48) X(64)
// The <DROP, MS, Q2, DET, OC> combinations the one-pass hs-32 backward is built for: plain, several KV streams, and
// the stage-2 epilogue with atomic or deterministic sums, each with Q / K / V read or made on chip
#define ATTN_FUSED32_OPS(X)                                                                        \
  X(false, false, false, false, false) X(true, false, false, false, false)                         \
  X(false, true, false, false, false) X(true, true, false, false, false)                           \
  X(false, false, true, false, false) X(true, false, true, false, false)                           \
  X(false, false, true, false, true) X(true, false, true, false, true)                             \
  X(false, false, true, true, false) X(true, false, true, true, false)                             \
  X(false, false, true, true, true) X(true, false, true, true, true)
// <DROP, depth> of the hs-64 ring forward, ring dQ pass and one-pass backward; <DROP, occ, depth> of the dK/dV ring
#define ATTN_RING64_FWD_OPS(X) X(false, 4) X(true, 4)
#define ATTN_RING64_DQ_OPS(X) X(false, 4) X(true, 4)
#define ATTN_RING64_DKDV_OPS(X) X(false, 2, 4) X(true, 2, 4) X(false, 3, 4) X(true, 3, 4)
#define ATTN_FUSED64_OPS(X) X(false, 3) X(true, 3)
// <DROP> of the on-chip-QKV hs-32 forward; tiles per wave of the mask kernel
#define ATTN_OC32_OPS(X) X(false) X(true)
#define ATTN_MASK_G(X) X(1) X(2) X(4) X(8) X(16)

// a launch as one switch key: the lists above become case labels (a doubled entry does not compile). `v`: hs of the
// chunked kernels, depth of the mmt_attn2.hip ones, g of the mask kernel
constexpr int attn_key(int family, int v, bool drop, bool ms = false, bool q2 = false, bool det = false,
                       bool oc = false, int occ = 0) {
  return family | (v << 4) | (drop ? 1 << 11 : 0) | (ms ? 1 << 12 : 0) | (q2 ? 1 << 13 : 0) | (det ? 1 << 14 : 0) |
         (oc ? 1 << 15 : 0) | (occ << 16);
}
inline int attn_key(const AttnLaunch& l) {
  const int v = l.family == ATTN_MASK ? l.g : l.family <= ATTN_CHUNK_DKDV ? l.hs : l.depth;
  return attn_key(l.family, v, l.drop, l.ms, l.q2, l.det, l.oc, l.occ);
}
constexpr bool attn_hs_built(int hs) {
#define X(h) || hs == h
  return false ATTN_CHUNK_HS(X);
#undef X
}
