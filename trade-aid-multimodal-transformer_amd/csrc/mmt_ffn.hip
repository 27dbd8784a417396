// One-launch FFN forward for gfx950 at C = 256 (round 8): the feed-forward block of a transformer layer
// (reference model.py:162-175, 225)
//   h   = relu(x W0^T + b0)            Linear(C, 4C) -> ReLU
//   out = resid + drop(h W2^T + b2)    Linear(4C, C) -> dropout -> residual add, + the next LayerNorm's forward
// A workgroup owns 128 rows and all 256 output columns and walks the 1024 hidden columns in 8 chunks of 128:
//  * the x tile (128 x 256 bf16) is loaded once by LDS-DMA and every wave keeps its 32 rows as stage-1 MFMA
//    fragments in registers (64 VGPRs): the 8 chunks re-read it at no LDS cost, and its 64 KiB go to the ring;
//  * per chunk, stage 1 is acc1 = W0[chunk] x^T over K = 256 (v_mfma_f32_32x32x16_bf16, hidden on accumulator
//    rows, 8 waves 4 (m) x 2 (n) of 32 rows x 64 hidden: ffn0's MFMA, K ascending, frag<> K-slot order), its
//    epilogue relu(acc1 + b0) -> bf16 -> the swizzled LDS h image (h_off), and stage 2 acc2 += W2[:, chunk]
//    h_chunk^T over K = 128 from that image (v_mfma_f32_16x16x32_bf16 with the ping-pong kernel's K slots, 64
//    rows x 64 columns per wave; acc2 lives across the whole walk: the 1024 K values ascending in one
//    accumulator, as gemm8_kernel's K loop adds them). Both products therefore give the two-launch path's bits;
//  * the weights stream as ONE sequence of 64 equal 16-KiB slices, two per step, through one ring of three
//    32-KiB slots (two steps = 64 KiB in flight): per chunk four W0 slices [128][64] then four W2 slices
//    [256][32], two LDS-DMA pieces per wave each, so the counted vmcnt pipeline never drains at a stage switch.
//    A step is one barrier and 16 (stage 1) or 32 (stage 2) MFMAs per wave, 32 steps per workgroup;
//  * the chunk's h rows leave for HBM (the backward reads them) from the image as row-major 16-B buffer stores,
//    two per thread in each of the chunk's two stage-2 steps. Stores and LDS-DMA loads share vmcnt in issue
//    order, so every thread issues every store (rows past M go out of the descriptor's range and are dropped)
//    and each step's wait counts them exactly (ffn_wait);
//  * b0 (4 KiB) sits in LDS from kernel start: a global load inside the walk would land between DMA pieces in
//    vmcnt order;
//  * the final epilogue is the shared epilogue_swap (bias, hash dropout, fp32 residual, bf16 copy, LayerNorm
//    forward on the owned rows), its staging tile in the ring.
// LDS: ring 96 + h 32 + b0 4 = 132 KiB, one workgroup per CU. Against ffn0 + ffn2 this removes the read
// of h (R x 4C x 2 B), one launch and one prologue / epilogue per row tile.
#include "mmt_gemm_dev.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int FFN_BM = 128;    // rows per workgroup
constexpr int FFN_C = 256;     // model width: K of stage 1, N of stage 2
constexpr int FFN_HID = 1024;  // hidden width
constexpr int FFN_CH = 128;    // hidden columns per chunk
constexpr int FFN_NCH = FFN_HID / FFN_CH;
constexpr int FFN_SLOT = 16384;  // one weight slice: W0 [128][64] or W2 [256][32] bf16
constexpr int FFN_DSLOT = 2 * FFN_SLOT;  // a step consumes two slices: one ring slot
constexpr int FFN_NS = 3;                // ring slots: 2 steps (4 slices, 64 KiB) in flight
constexpr int FFN_RING = FFN_NS * FFN_DSLOT;
constexpr int FFN_NSTEP = FFN_NCH * 4;
constexpr int FFN_HPITCH = FFN_CH * 2;
constexpr int FFN_HIMG = FFN_BM * FFN_HPITCH;
constexpr int FFN_LDS = FFN_RING + FFN_HIMG + FFN_HID * 4;
constexpr int FFN_EPI_ROWS = 32;
using FfnT2 = TileCfg<2, 4, 2, 2>;  // stage-2 / epilogue geometry: 128 x 256, waves 2 (m) x 4 (n)
static_assert(FFN_EPI_ROWS * (FfnT2::BN + 4) * 4 <= FFN_RING, "the epilogue's staging tile reuses the ring");
static_assert(FFN_BM * FFN_C * 2 <= (FFN_NS - 1) * FFN_DSLOT, "the x tile is staged in ring slots 1..2");
static_assert(FFN_LDS <= 160 * 1024, "LDS per workgroup");

// h image: row m, 16-B chunk c (8 hidden columns) at m * pitch + ((c ^ (m & 15)) * 16) (as mlp2_kernel's)
__device__ __forceinline__ int h_off(int m, int chunk) { return m * FFN_HPITCH + ((chunk ^ (m & 15)) << 4); }

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// (the s_nop: the data registers may be rewritten right after; the compiler does not see inside the asm)
__device__ __forceinline__ void store16(const i32x4& rsrc, int voff, u32x4 v) {
  asm volatile("buffer_store_dwordx4 %0, %1, %2, 0 offen\n\ts_nop 1" : : "v"(v), "v"(voff), "s"(rsrc) : "memory");
}

// outstanding vmcnt operations step I (chunk c, position d) may leave in flight when it waits for its two
// slices (issue order after their 4 pieces): the h stores of step I - 2 (two per stage-2 step, d >= 2), the next
// step's 4 pieces, the h stores of step I - 1
constexpr int ffn_wait(int c, int d) {
  const int i = 4 * c + d;
  int n = i + 1 < FFN_NSTEP ? 4 : 0;
  for (int j = i - 2; j < i; ++j)
    if (j >= 0 && (j & 3) >= 2) n += 2;
  return n;
}

}  // namespace

__global__ __launch_bounds__(512, 1) void ffn_fwd_kernel(Mlp2Batch batch) {
  constexpr int NW = 8;
  __shared__ __attribute__((aligned(1024))) char lds[FFN_LDS];
  char* const himg = lds + FFN_RING;
  float* const b0s = reinterpret_cast<float*>(himg + FFN_HIMG);

  const int prob = blockIdx.z;
  const GemmProblem& P1 = batch.g1[prob];
  const GemmProblem& P2 = batch.g2[prob];
  const int M = __builtin_amdgcn_readfirstlane(P1.M);
  const int ntiles = (M + FFN_BM - 1) / FFN_BM;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  if (tile >= ntiles) return;
  const int m0 = tile * FFN_BM;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;    // stage 2: 2 (m) x 4 (n) waves of 64 rows x 64 columns
  const int wm1 = wave >> 1, wn1 = wave & 1;  // stage 1: 4 (m) x 2 (n) waves of 32 rows x 64 hidden
  const int h = lane >> 5, r = lane & 31;     // 32x32x16 lane map (stage 1)
  const int g16 = lane >> 4, l16 = lane & 15;  // 16x16x32 lane map (stage 2)

  const int ldx = __builtin_amdgcn_readfirstlane(P1.lda), ldw0 = __builtin_amdgcn_readfirstlane(P1.ldb);
  const int ldw2 = __builtin_amdgcn_readfirstlane(P2.ldb), ldh = __builtin_amdgcn_readfirstlane(P1.ldo16);
  const bf16_t* const W0p = sgpr_ptr(P1.B);
  const i32x4 rx = op_rsrc<true>(P1.A, ldx, M, FFN_C, m0, 0);
  const i32x4 rw2 = op_rsrc<true>(P2.B, ldw2, FFN_C, FFN_HID, 0, 0);
  // h rows of this tile: rows past M lie beyond the range and their stores are dropped
  const i32x4 rh = make_rsrc(reinterpret_cast<const char*>(P1.o16) + (int64_t)m0 * ldh * 2, (int64_t)(M - m0) * ldh * 2);

  // step (chunk c, position d) consumes two 16-KiB slices, side by side in one ring slot: d 0, 1 = W0 rows
  // [128 c, +128) x K [128 d, +64) and [128 d + 64, +64); d 2, 3 = W2 x K [128 c + 64 (d - 2), +32) and the next 32
  auto issue = [&](int slot, int c, auto DC) {
    constexpr int D = decltype(DC)::value;
    char* st = lds + slot * FFN_DSLOT;
    if constexpr (D < 2) {
      const i32x4 rw0 = op_rsrc<true>(W0p, ldw0, FFN_HID, FFN_C, c * FFN_CH, 0);
      issue_tile<64, true, FFN_CH, NW>(rw0, st, ldw0, FFN_HID, FFN_C, c * FFN_CH, 128 * D, wave, lane);
      issue_tile<64, true, FFN_CH, NW>(rw0, st + FFN_SLOT, ldw0, FFN_HID, FFN_C, c * FFN_CH, 128 * D + 64, wave, lane);
    } else {
      issue_tile<32, true, FFN_C, NW>(rw2, st, ldw2, FFN_C, FFN_HID, 0, c * FFN_CH + 64 * (D - 2), wave, lane);
      issue_tile<32, true, FFN_C, NW>(rw2, st + FFN_SLOT, ldw2, FFN_C, FFN_HID, 0, c * FFN_CH + 64 * (D - 2) + 32, wave, lane);
    }
  };

  // prologue: the x tile (four [128][64] images, 8 pieces per wave) into ring slots 1..2 and step 0's slices
  // into slot 0, b0 into LDS; then every wave takes its 32 rows of x into registers as stage-1 fragments (the
  // tile is read 8 times, once per chunk: from registers that costs no LDS bandwidth and frees 64 KiB for the
  // ring) and step 1's slices follow into slot 1
  char* const xst = lds + FFN_DSLOT;
#pragma unroll
  for (int t = 0; t < 4; ++t) issue_tile<64, true, FFN_BM, NW>(rx, xst + t * 16384, ldx, M, FFN_C, m0, 64 * t, wave, lane);
  issue(0, 0, std::integral_constant<int, 0>{});
  {
    const float2 bv = *reinterpret_cast<const float2*>(P1.bias + 2 * tid);
    *reinterpret_cast<float2*>(b0s + 2 * tid) = bv;
  }
  wait_vm(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  bf16x8 xr[16];  // [K step of 16]: rows wm1 32 + r
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s) xr[4 * t + s] = frag<64, true, FFN_BM>(xst + t * 16384, wm1 * 32, s, lane);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // every wave's reads of the staged x are done: slots 1..2 are free
  issue(1, 0, std::integral_constant<int, 1>{});

  f32x16 acc1[2];
  f32x4 acc2[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc2[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Step I (chunk c, position D, slot I % 3): wait for its slices (ffn_wait: the next step's pieces and the h
  // stores issued since stay in flight), barrier (they landed for every wave, every wave's reads of step I - 1
  // are done), issue step I + 2's slices into step I - 1's slot, [stage 2: two h stores], the MFMAs, [D == 1: the
  // stage-1 epilogue into the h image, published by the next step's barrier]. The counts differ from the steady
  // state only in the first chunk (no stores behind) and the last (nothing ahead), so the chunk loop peels those.
  auto step = [&](int c, int slot, auto DC, auto KC) {
    constexpr int D = decltype(DC)::value;
    constexpr int KIND = decltype(KC)::value;  // 0 first chunk, 1 steady, 2 last chunk
    constexpr int CREP = KIND == 0 ? 0 : KIND == 1 ? 1 : FFN_NCH - 1;
    static_assert(ffn_wait(1, D) == ffn_wait(FFN_NCH - 2, D), "steady-state counts");
    wait_vm(ffn_wait(CREP, D));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    u32x4 hv[2];
    int hvoff[2];
    if constexpr (D >= 2) {  // this thread's 2 x 16 B of the chunk's h rows: pieces 2 (D - 2), + 1 of four
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int idx = (2 * (D - 2) + u) * 512 + tid;
        const int m = idx >> 4, cc = idx & 15;
        hv[u] = *reinterpret_cast<const u32x4*>(himg + h_off(m, cc));
        hvoff[u] = m0 + m < M ? (m * ldh + c * FFN_CH + 8 * cc) * 2 : 0x7fffffff;
      }
    }
    const int nslot = slot == 0 ? FFN_NS - 1 : slot - 1;  // (slot + 2) % 3
    if constexpr (D < 2) issue(nslot, c, std::integral_constant<int, D + 2>{});
    else if constexpr (KIND != 2) issue(nslot, c + 1, std::integral_constant<int, D - 2>{});
    if constexpr (D >= 2) {
      store16(rh, hvoff[0], hv[0]);
      store16(rh, hvoff[1], hv[1]);
    }
    if constexpr (D < 2) {
      if constexpr (D == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc1[i][e] = 0.f;
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const char* imgW = lds + slot * FFN_DSLOT + q * FFN_SLOT;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          bf16x8 fb[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) fb[i] = frag<64, true, FFN_CH>(imgW, wn1 * 64 + 32 * i, s, lane);
#pragma unroll
          for (int i = 0; i < 2; ++i) acc1[i] = mfma32(fb[i], xr[8 * D + 4 * q + s], acc1[i]);
        }
      }
      if constexpr (D == 1) {
        // h = relu(acc1 + b0) -> bf16 -> the image (lane (r, h) holds row m = wm1 32 + r, hidden
        // n = wn1 64 + 32 i + 8 g + 4 h + e of the chunk): ffn0's epilogue arithmetic
        const int m = wm1 * 32 + r;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(b0s + c * FFN_CH + wn1 * 64 + 32 * i + 8 * g + 4 * h);
            const uint32_t lo = pack2bf(fmaxf(acc1[i][4 * g] + bv[0], 0.0f), fmaxf(acc1[i][4 * g + 1] + bv[1], 0.0f));
            const uint32_t hi = pack2bf(fmaxf(acc1[i][4 * g + 2] + bv[2], 0.0f), fmaxf(acc1[i][4 * g + 3] + bv[3], 0.0f));
            *reinterpret_cast<u32x2*>(himg + h_off(m, wn1 * 8 + 4 * i + g) + 8 * h) = u32x2{lo, hi};
          }
      }
    } else {
      // 16x16x32 fragments: lane holds row (l16) and k = 8 g16 + 0..7 of a slice's 32
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const char* imgW = lds + slot * FFN_DSLOT + q * FFN_SLOT;
        bf16x8 xf[4], wf[4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
          xf[mb] = *reinterpret_cast<const bf16x8*>(himg + h_off(wm * 64 + 16 * mb + l16, 4 * (2 * (D - 2) + q) + g16));
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          const int row = wn * 64 + 16 * nb + l16;
          wf[nb] = *reinterpret_cast<const bf16x8*>(imgW + row * 64 + kc_swz<32>(g16, row) * 16);
        }
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
          for (int mb = 0; mb < 4; ++mb) acc2[nb][mb] = mfma16(wf[nb], xf[mb], acc2[nb][mb]);
      }
    }
  };

  int slot = 0;
  auto chunk = [&](int c, auto KC) {
    auto next = [&] { slot = slot == FFN_NS - 1 ? 0 : slot + 1; };
    step(c, slot, std::integral_constant<int, 0>{}, KC); next();
    step(c, slot, std::integral_constant<int, 1>{}, KC); next();
    step(c, slot, std::integral_constant<int, 2>{}, KC); next();
    step(c, slot, std::integral_constant<int, 3>{}, KC); next();
  };
  chunk(0, std::integral_constant<int, 0>{});
#pragma unroll 1
  for (int c = 1; c < FFN_NCH - 1; ++c) chunk(c, std::integral_constant<int, 1>{});
  chunk(FFN_NCH - 1, std::integral_constant<int, 2>{});

  // every DMA piece has landed (the last wait left only h stores in flight); the epilogue's first barrier
  // closes the last slices' reads before its staging tile overwrites the ring
  epilogue_swap<FfnT2, EPI_BIAS_RESID_F32, FFN_EPI_ROWS>(P2, acc2, lds, P2.o32, P2.alpha, m0, 0, tid, lane, wave);
}

// a field the kernel does not implement must be unset (as mlp2_unused_clear): the engine then runs ffn0 + ffn2
static bool ffn_unused_clear(const GemmProblem& p1, const GemmProblem& p2) {
  for (const GemmProblem* p : {&p1, &p2})
    if (p->o8 || p->s8 || p->mask8 || p->qkv2_out || p->qkv2_h1_only || p->split_stride || p->sa || p->sb ||
        p->ln_dgamma || p->ln_dbeta || p->ln_gamma || p->aux || p->dbias || p->alpha_ptr)
      return false;
  return !p1.resid && !p1.o32 && !p1.drop_thr && !p1.lnf_y && !p1.lnf_gamma && !p1.lnf_beta && !p1.lnf_mean &&
         !p1.lnf_rstd;
}

bool mmt_ffn_ok(const Mlp2Batch& b) {
  if (b.count <= 0 || b.count > MMT_MLP2_GROUP) return false;
  for (int g = 0; g < b.count; ++g) {
    const GemmProblem& p1 = b.g1[g];
    const GemmProblem& p2 = b.g2[g];
    if (p1.N != FFN_HID || p1.K != FFN_C || p2.N != FFN_C || p2.K != FFN_HID || p2.M != p1.M || p1.M < 1) return false;
    if (!p1.A || !p1.B || !p1.bias || !p1.o16 || !p2.B || !p2.bias || !p2.resid || !p2.o32) return false;
    if (p2.A != p1.o16 || p2.lda != p1.ldo16) return false;  // stage 2 reads the h this launch makes
    if ((p1.lda & 7) || (p1.ldb & 7) || (p2.ldb & 7) || (p1.ldo16 & 7) || (p2.ldc & 3) || (p2.ldres & 3) ||
        (p2.o16 && ((p2.ldo16 & 7) || p2.ldo16 < FFN_C)) || p1.lda < FFN_C || p1.ldb < FFN_C || p2.ldb < FFN_HID ||
        p1.ldo16 < FFN_HID || p2.ldc < FFN_C || p2.ldres < FFN_C)
      return false;
    if (((uintptr_t)p1.A | (uintptr_t)p1.B | (uintptr_t)p2.B | (uintptr_t)p1.o16 | (uintptr_t)p2.o32 |
         (uintptr_t)p2.resid | (uintptr_t)p1.bias | (uintptr_t)p2.bias | (uintptr_t)p2.o16) & 15)
      return false;
    if (!ffn_unused_clear(p1, p2)) return false;
    if (p1.alpha != 1.0f || p2.alpha != 1.0f) return false;
    // 32-bit buffer offsets: a descriptor spans at most 256 rows of its operand
    if ((int64_t)513 * std::max(std::max(p1.lda, p1.ldb), std::max(p2.ldb, p1.ldo16)) * 2 >= ((int64_t)1 << 31)) return false;
    const bool any = p2.lnf_y || p2.lnf_gamma || p2.lnf_beta || p2.lnf_mean || p2.lnf_rstd;
    const bool all = p2.lnf_y && p2.lnf_gamma && p2.lnf_beta && p2.lnf_mean && p2.lnf_rstd;
    if (any && (!all || (((uintptr_t)p2.lnf_y | (uintptr_t)p2.lnf_gamma | (uintptr_t)p2.lnf_beta) & 15))) return false;
  }
  return true;
}

hipError_t mmt_launch_ffn(const Mlp2Batch& b, hipStream_t s) {
  if (!mmt_ffn_ok(b)) return hipErrorInvalidValue;
  int mt = 0;
  for (int g = 0; g < b.count; ++g) mt = std::max(mt, (b.g1[g].M + FFN_BM - 1) / FFN_BM);
  hipLaunchKernelGGL(ffn_fwd_kernel, dim3(mt, 1, b.count), dim3(512), 0, s, b);
  return hipGetLastError();
}
