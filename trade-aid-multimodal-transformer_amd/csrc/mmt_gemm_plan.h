// The GEMM launch plan (host only): which kernel a GemmBatch takes, with which template arguments and grid.
// mmt_gemm_plan (mmt_gemm.hip) fills one for every launcher; the launchers launch what it says, the engine
// and the tests read it. It calls no HIP runtime function and allocates nothing.
#pragma once
#include "mmt_kernels.h"

enum GemmKind {       // the launcher that asks
  GEMM_LINEAR = 0,    // mmt_launch_gemm
  GEMM_WGRAD,         // mmt_launch_gemm_wgrad
  GEMM_RESID_LN,      // mmt_launch_gemm_resid_ln
  GEMM_LN_BWD,        // mmt_launch_gemm_ln_bwd
  GEMM_F8             // mmt_launch_gemm_f8
};
enum GemmPlanStatus { GEMM_PLAN_OK = 0, GEMM_PLAN_EMPTY /* nothing to launch */, GEMM_PLAN_INVALID };
enum GemmFamily { GEMM_RING = 0 /* gemm_kernel */, GEMM_PINGPONG /* gemm8_kernel */, GEMM_FP8 /* gemm_f8_kernel */ };
enum GemmTile { GEMM_TILE_128 = 0, GEMM_TILE_128x256, GEMM_TILE_256, GEMM_TILE_128x512 };

struct GemmPlan {
  int status;              // GemmPlanStatus; the rest is meaningful when OK. tile is also set when the plan is EMPTY or
                           // INVALID, unless the batch has no problem or the (layouts, epilogue) pair is not built (then 0)
  int family, tile;        // GemmFamily, GemmTile
  int bk, stages, minb;    // K-step, LDS stages, minimum blocks per CU (__launch_bounds__)
  int swap;                // C^T tiles (vector epilogue stores); 0: N on lanes (the atomic epilogue)
  int a_kc, b_kc, epi;     // the kernel's operand layouts and epilogue (weight gradients: ACC or STORE)
  int gx, gy, gz;          // grid: tiles of the largest problem, K slices, problems
  // split-K weight gradients: 0 = one K pass accumulating in place, 1 = gy slabs + a reduce launch of
  // reduce_blocks x gz workgroups; xcd_plane = GemmBatch::xcd_plane of the launch
  int slabs, reduce_blocks, xcd_plane;
};
constexpr int GEMM_PLAN_INTS = sizeof(GemmPlan) / sizeof(int);  // mmt_op_gemm_plan writes them in this order

// The operand layouts and the epilogue a kind fixes (GEMM_LINEAR: none; GEMM_F8: the layouts; the weight gradient's
// epilogue becomes ACC or STORE with the split-K factor): the one place that says so.
inline void gemm_kind_ops(int kind, bool& a_kc, bool& b_kc, int& epi) {
  if (kind == GEMM_WGRAD) { a_kc = b_kc = false; epi = EPI_STORE_F32; }
  if (kind == GEMM_RESID_LN) { a_kc = b_kc = true; epi = EPI_BIAS_RESID_F32; }
  if (kind == GEMM_LN_BWD) { a_kc = true; b_kc = false; epi = EPI_LN_BWD_F32; }
  if (kind == GEMM_F8) a_kc = b_kc = true;
}

// a_kc, b_kc, epi: read only where the kind leaves them open (gemm_kind_ops). splits: split-K factor of the atomic /
// fp32-store launches with MN-contiguous A (<= 0: automatic for the atomic ones); slab_bytes: the weight gradients'
// slab capacity (0: no slab). Both ignored by the other kinds.
GemmPlan mmt_gemm_plan(const GemmBatch& b, int kind, bool a_kc = true, bool b_kc = true, int epi = 0, int splits = 1,
                       int64_t slab_bytes = 0);

// The (A K-contiguous, B K-contiguous, SWAP, epilogue) combinations the ring kernel is built for: forward,
// backward data, weight gradient (split-K: atomic with N on lanes, or slabs / accumulate), dX^T products.
#define GEMM_RING_OPS(X)                                                                                        \
  X(true, true, true, EPI_STORE_BF16) X(true, true, true, EPI_BIAS_TANH_BF16) X(true, true, true, EPI_BIAS_RELU_BF16) \
  X(true, true, true, EPI_BIAS_RESID_F32) X(true, true, true, EPI_STORE_F32) X(true, true, true, EPI_ACC_F32)    \
  X(true, false, true, EPI_STORE_BF16) X(true, false, true, EPI_DTANH_BF16) X(true, false, true, EPI_DRELU_BF16) \
  X(true, false, true, EPI_STORE_F32) X(true, false, true, EPI_ACC_F32)                                          \
  X(false, false, false, EPI_ATOMIC_F32) X(false, false, true, EPI_STORE_F32) X(false, false, true, EPI_ACC_F32) \
  X(false, true, false, EPI_ATOMIC_F32) X(false, true, true, EPI_STORE_F32)
// ... and the one more the row-wide launches add (256 x 256 BK 64 x 2 and 128 x 512 only)
#define GEMM_RING_LN_BWD_OP(X) X(true, false, true, EPI_LN_BWD_F32)
// The (A K-contiguous, B K-contiguous, epilogue) combinations mmt_gemm8.hip instantiates (all SWAP)
#define GEMM8_OPS(X)                                                                                    \
  X(true, true, EPI_STORE_BF16) X(true, true, EPI_BIAS_TANH_BF16) X(true, true, EPI_BIAS_RELU_BF16)      \
  X(true, true, EPI_BIAS_RESID_F32) X(true, true, EPI_STORE_F32) X(true, true, EPI_ACC_F32)              \
  X(true, false, EPI_LN_BWD_F32) X(true, false, EPI_STORE_BF16) X(true, false, EPI_DTANH_BF16)           \
  X(true, false, EPI_DRELU_BF16) X(true, false, EPI_STORE_F32) X(true, false, EPI_ACC_F32)               \
  X(false, false, EPI_STORE_F32) X(false, false, EPI_ACC_F32)
// The epilogues of the MX-fp8 kernel (both operands K-contiguous, SWAP)
#define GEMM_F8_OPS(X) \
  X(EPI_STORE_BF16) X(EPI_BIAS_TANH_BF16) X(EPI_BIAS_RELU_BF16) X(EPI_BIAS_RESID_F32) X(EPI_STORE_F32)

// (layouts, epilogue) as one switch key: the lists above become case labels (a doubled entry does not compile)
constexpr int gemm_op_key(bool akc, bool bkc, int epi) { return (epi << 2) | (bkc ? 2 : 0) | (akc ? 1 : 0); }
constexpr bool gemm8_supports(bool akc, bool bkc, int epi) {
#define X(a, b, e) || (akc == a && bkc == b && epi == e)
  return false GEMM8_OPS(X);
#undef X
}

// launches the plan's ping-pong kernel (mmt_gemm8.hip); hipErrorInvalidValue outside GEMM8_OPS
hipError_t mmt_launch_gemm8(const GemmBatch& b, const GemmPlan& p, hipStream_t s);
