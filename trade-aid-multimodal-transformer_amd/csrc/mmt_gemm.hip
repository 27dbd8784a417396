// bf16 MFMA GEMM for gfx950 with fused epilogues (forward linear, backward data, weight grad).
//
// Tile 128x128, K-step 64, 256 threads = 4 waves (2x2), each wave a 64x64 sub-tile as 2x2
// v_mfma_f32_32x32x16_bf16 accumulators (fp32).
//
// Operand staging is direct global->LDS (buffer_load_dwordx4 ... lds), no VGPR round trip, into
// an S-stage LDS ring: the loads of K-step t+S-1 are in flight while step t computes; each step
// starts with a counted `s_waitcnt vmcnt` (never 0 while later stages are in flight) and one raw
// s_barrier. Out-of-range chunks (M/N/K edges) get an out-of-bounds buffer offset and land as
// zeros (the buffer descriptor's range check), so edge tiles need no branches.
//   K-contiguous operand  -> image [128 rows][64 k], 128-B rows, 16-B chunk XOR swizzle
//                            chunk ^= (row>>1)&7 (conflict-free ds_read_b128 fragments)
//   MN-contiguous operand -> image [64 k][128], 256-B rows, chunk ^= (k&3)<<2 (conflict-free
//                            ds_read_b64_tr_b16 transposed fragments)
// The swizzle is applied on the per-lane GLOBAL source address (the LDS destination of an
// LDS-DMA is lane-linear) and again on the fragment read.
// SWAP=true computes C^T tiles (N on accumulator rows, M on lanes): each lane owns one output row
// and 4 consecutive columns per register group -> 8/16-B vector epilogue stores.
// SWAP=false keeps N on lanes: 32 lanes hit 128 contiguous bytes of one row, the shape fp32
// atomics need (weight-grad split-K accumulate).
#include "mmt_common.h"
#include "mmt_kernels.h"

#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "mmt_gemm_dev.h"
#include "mmt_gemm_plan.h"


// Diagnostic timestamps (-DMMT_GEMM_STAMPS builds only; tools/gemm_stamps.py): thread 0 of each block
// records s_memtime at phase boundaries into batch.stamps[block * 8 + k]: 0 start, 1 prologue issued,
// 2 first K-step's stage landed (after its barrier), 3 K loop done, 4 epilogue done, 5 HW_ID, 6 XCC_ID.
#ifdef MMT_GEMM_STAMPS
static unsigned long long* g_stamps = nullptr;
extern "C" int mmt_gemm_set_stamps(void* p) { g_stamps = (unsigned long long*)p; return 0; }
#define GEMM_STAMP(k)                                                                                   \
  do {                                                                                                \
    if (batch.stamps && threadIdx.x == 0)                                                             \
      batch.stamps[((size_t)blockIdx.z * gridDim.y * gridDim.x + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + (k)] = \
          (k) == 5   ? (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11))  \
          : (k) == 6 ? (unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) \
                     : (unsigned long long)__builtin_amdgcn_s_memtime();                             \
  } while (0)
#else
#define GEMM_STAMP(k) \
  do {                \
  } while (0)
#endif


// Per-head Q/K/V stage 2 fused into the stage-1 GEMM's epilogue (reference model.py:36-50,
// each head's key / query / value = Linear(hs/2, hs, no bias) of tanh(Linear(C, hs/2))). acc holds
// this wave's TN x TM 32x32 sub-tiles of h1^T (stage-1 column n on accumulator rows, row m on lanes).
// First, in place, acc = h1 = tanh(alpha acc + bias) (what the epilogue then stores as o16, PRE).
// Each hh-wide column block blk of h1 (hh = 16 or 32) is one head's K, Q or V stage-1 output; its
// stage 2 out[m][blk*2hh + o] = sum_k W2[blk][o][k] h1[m][blk*hh + k] runs on MFMA straight from
// the accumulator registers: lane (r, h) holds h1[r][4h + 0..3] and h1[r][8 + 4h + 0..3] of a
// 16-column block (accumulator groups g and g + 1), which is a K-16 B operand with K permuted
// (slot j <-> k = 4h + j, j < 4; 8 + 4h + j - 4, j >= 4) -- the W2 fragment takes the same
// permutation. A 32 x 32 stage-1 sub-tile yields 64 consecutive output columns (2 n0 + ...) of 32
// rows: they cross a wave-private LDS slot (no block barrier) so they leave as 128-B row segments,
// 8 rows per store instruction (storing the MFMA layout directly touches 32 rows x 32 B per store
// and ran the target's qkv1 launch 169 us against 78 + 65 for the unfused pair).
// The W2 fragments of the tile's stage-1 column blocks, converted to bf16 and permuted once per block
// into LDS at kernel start (before the K loop; the epilogue reads them with one ds_read_b128 each):
// fragment (b, ot, kh) of local block b = lane-ordered 16-B pieces at ((b * 2 + ot) * 2 + kh) KiB
// (HH = 16: ot = kh = 0, fragment b at b KiB). Fetching them from global fp32 inside the epilogue
// put two dependent global loads in front of every sub-tile's MFMAs.
constexpr int QKV2_W2_LDS = 16384;
template <class TL>
__device__ __forceinline__ void qkv2_stage_w2(const GemmProblem& P, char* w2l, int n0, int tid) {
  const int HH = P.qkv2_hh, HS = 2 * HH;
  const int nfrag = HH == 32 ? (TL::BN / 32) * 4 : TL::BN / 16;  // 16 (HH 32) or 8 (HH 16)
  const int blk0 = n0 / HH, nblk = P.N / HH;
  for (int q = tid; q < nfrag * 64; q += TL::NT) {
    const int f = q >> 6, ln = q & 63, r = ln & 31, h = ln >> 5;
    const int b = HH == 32 ? f >> 2 : f, ot = HH == 32 ? (f >> 1) & 1 : 0, kh = HH == 32 ? f & 1 : 0;
    u32x4 u = {0u, 0u, 0u, 0u};
    if (blk0 + b < nblk) {
      const float* w = P.qkv2_w2 + ((int64_t)(blk0 + b) * HS + ot * 32 + r) * HH + 16 * kh + 4 * h;
      const f32x4 lo = *reinterpret_cast<const f32x4*>(w);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(w + 8);
      u = u32x4{pack2bf(lo[0], lo[1]), pack2bf(lo[2], lo[3]), pack2bf(hi[0], hi[1]), pack2bf(hi[2], hi[3])};
    }
    *reinterpret_cast<u32x4*>(w2l + f * 1024 + ln * 16) = u;
  }
}

template <class TL>
__device__ __forceinline__ void qkv2_fused(const GemmProblem& P, f32x16 (&acc)[TL::TN][TL::TM], char* lds, char* w2l,
                                           float alpha, int m0, int n0, int lane, int wave) {
  constexpr int TM = TL::TM, TN = TL::TN;
  constexpr int SROW = 144;  // slot row pitch (128 B of bf16 + 16 B pad)
  const int wm = wave / TL::WN, wn = wave % TL::WN;
  const int h = lane >> 5, r = lane & 31;
  const int M = P.M, N = P.N, HH = P.qkv2_hh, HS = 2 * HH;
  const int nw = n0 + wn * TN * 32;  // first stage-1 column of this wave
  char* slot = lds + wave * 32 * SROW;
  // W2 fragment of block blk, output tile ot, K-16 half kh (HH = 32: two halves): lane (o, h), slot j
  // (staged in LDS by qkv2_stage_w2)
  const int blk0 = n0 / HH;
  auto w2frag = [&](int blk, int ot, int kh) {
    const int f = HH == 32 ? ((blk - blk0) * 2 + ot) * 2 + kh : blk - blk0;
    return *reinterpret_cast<const bf16x8*>(w2l + f * 1024 + lane * 16);
  };
  // accumulator elements [8q, 8q + 8) of a sub-tile as a bf16 B operand (16 columns of h1)
  auto hfrag = [&](const f32x16& a, int q) {
    const u32x4 u = {pack2bf(a[8 * q], a[8 * q + 1]), pack2bf(a[8 * q + 2], a[8 * q + 3]),
                     pack2bf(a[8 * q + 4], a[8 * q + 5]), pack2bf(a[8 * q + 6], a[8 * q + 7])};
    return __builtin_bit_cast(bf16x8, u);
  };
  // D[o][m] (32 output columns c0 + o of the sub-tile's 64, rows m = lanes) into the slot: 16-B row
  // pieces after a v_permlane32_swap of the two halves
  auto put = [&](const f32x16& d, int c0) {
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const int ga = 2 * pr, gb = 2 * pr + 1;
      const auto s0 = __builtin_amdgcn_permlane32_swap(pack2bf(d[4 * ga], d[4 * ga + 1]), pack2bf(d[4 * gb], d[4 * gb + 1]),
                                                       false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(pack2bf(d[4 * ga + 2], d[4 * ga + 3]),
                                                       pack2bf(d[4 * gb + 2], d[4 * gb + 3]), false, false);
      *reinterpret_cast<u32x4*>(slot + r * SROW + (c0 + 16 * pr + 8 * h) * 2) = u32x4{s0[0], s1[0], s0[1], s1[1]};
    }
  };
  // the slot's 32 rows x 64 columns to out[m0j + row][2 nb + col]: 8 rows of 128 B per store
  auto drain = [&](int nb, int j) {
    const int mj = m0 + wm * TM * 32 + 32 * j;
    const int cc = (lane & 7) * 8, cg = 2 * nb + cc;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = 8 * it + (lane >> 3);
      const u32x4 v = *reinterpret_cast<const u32x4*>(slot + row * SROW + cc * 2);
      if (mj + row < M && cg < 2 * N)
        *reinterpret_cast<u32x4*>(P.qkv2_out + (int64_t)(mj + row) * P.qkv2_ld + cg) = v;
    }
  };
  f32x16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  __syncthreads();  // the slots overlay the stage ring: every wave's last K-step reads are done
  // one 32x32 sub-tile at a time (activation, then its stage-2 MFMAs, slot, stores): every value is
  // produced right before its use, so the epilogue stays inside the main loop's register budget
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    const int nb = nw + 32 * i;
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      // (the bias is already in the accumulators: gemm_kernel starts them at bias / alpha)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = fast_tanh(alpha * acc[i][j][e]);
      if (nb < N) {
        if (HH == 16) {
#pragma unroll
          for (int q = 0; q < 2; ++q)
            if (nb + 16 * q < N) put(mfma32(w2frag((nb + 16 * q) / 16, 0, 0), hfrag(acc[i][j], q), z), 32 * q);
        } else {  // HH == 32: K = 32 in two halves, two output tiles
          const bf16x8 h0 = hfrag(acc[i][j], 0), h1 = hfrag(acc[i][j], 1);
#pragma unroll
          for (int ot = 0; ot < 2; ++ot) put(mfma32(w2frag(nb / 32, ot, 1), h1, mfma32(w2frag(nb / 32, ot, 0), h0, z)), 32 * ot);
        }
        drain(nb, j);  // (LDS ops of one wave complete in order: the next put cannot pass these reads)
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}


// MINB > 1 (128x128 tile only): a launch-bounds hint of MINB blocks per CU, with the epilogue staged in
// 64-row passes so the LDS footprint leaves room for them (variants 5 and 6)
template <class TL, int BK, int ST, bool A_KC, bool B_KC, bool SWAP, int EPI, int MINB = 1>
__global__ __launch_bounds__(TL::NT, MINB) void gemm_kernel(GemmBatch batch) {
  constexpr int GBM = TL::BM, GBN = TL::BN, NW = TL::NW, NT = TL::NT, TM = TL::TM, TN = TL::TN;
  constexpr int IMG_A = GBM * BK * 2, IMG_B = GBN * BK * 2;  // per operand per stage (both layouts)
  constexpr int STAGE_BYTES = IMG_A + IMG_B;
  constexpr int PIECES = (GBM + GBN) * BK / 512 / NW;        // LDS-DMA pieces per wave per stage (A + B)
  constexpr int AI = SWAP ? TN : TM, AJ = SWAP ? TM : TN;    // accumulator sub-tile grid
  // XCD-aware remap (bijective): blocks b and b+8 share an XCD; give each XCD a contiguous run
  // of tiles so neighbouring tiles (same A row panel) share that XCD's L2
  int tile = blockIdx.x;
  int split = blockIdx.y;
  int prob = blockIdx.z;
  const int nsplit = gridDim.y;
  if (batch.xcd_plane) {
    // weight gradients: remap the whole (tile, split, problem) grid XCD-major, so the tiles of one
    // (K slice, problem) -- which share its dY / X panels -- run on one XCD's L2 instead of being
    // spread over the eight (C1: dW fetch bytes per launch 214 -> 166 MB)
    const int nwg = gridDim.x * nsplit * gridDim.z;
    const int lin = blockIdx.x + gridDim.x * (blockIdx.y + nsplit * blockIdx.z);
    const int x = lin % 8, q = nwg / 8, rr = nwg % 8;
    const int l2 = (x < rr ? x * (q + 1) : rr * (q + 1) + (x - rr) * q) + lin / 8;
    tile = l2 % gridDim.x;
    split = (l2 / gridDim.x) % nsplit;
    prob = l2 / (gridDim.x * nsplit);
  }
  const GemmProblem& P = batch.p[prob];
  // (readfirstlane: values the compiler cannot rematerialise by re-loading the kernel argument; as plain
  // P.* reads it re-loaded lda in front of every K-step's DMA, an s_load plus a full lgkmcnt wait)
  const int M = __builtin_amdgcn_readfirstlane(P.M), N = __builtin_amdgcn_readfirstlane(P.N);
  const int K = __builtin_amdgcn_readfirstlane(P.K);
  const int tiles_n = (N + GBN - 1) / GBN;
  const int tiles_m = (M + GBM - 1) / GBM;
  const int ntiles = tiles_m * tiles_n;
  if (!batch.xcd_plane) {
    const int nwg = gridDim.x;
    const int x = tile % 8, q = nwg / 8, rr = nwg % 8;
    tile = (x < rr ? x * (q + 1) : rr * (q + 1) + (x - rr) * q) + tile / 8;
  }
  if (tile >= ntiles) return;
  GEMM_STAMP(0);
  GEMM_STAMP(5);
  GEMM_STAMP(6);
  const int tm = tile / tiles_n, tn = tile % tiles_n;
  const int m0 = tm * GBM, n0 = tn * GBN;
  const int ksteps = (K + BK - 1) / BK;
  const int kper = (ksteps + nsplit - 1) / nsplit;
  const int ks0 = split * kper;
  const int ks1 = min(ksteps, ks0 + kper);
  if (EPI == EPI_ATOMIC_F32 && ks0 >= ks1) return;  // nothing to add (a slab split still writes its zeros)

  // one LDS array (a second __shared__ object can make hipcc drain vmcnt before ds_reads):
  // the stage ring during the K loop, the fp32 output tile (EPI_ROWS x (GBN + 4)) in the epilogue
  constexpr int EPI_ROWS = (GBN >= 512 || (GBM == 128 && GBN == 256)) ? 32 : (GBM == 128 && MINB == 1) ? 128 : 64;
  constexpr int RING = ST * STAGE_BYTES, CTILE = EPI_ROWS * (GBN + 4) * 4;
  constexpr int LDS_MAIN = RING > CTILE ? RING : CTILE;
  // + the fused Q/K/V stage 2's W2 fragments (qkv2_stage_w2)
  constexpr int LDS_W2 = (SWAP && EPI == EPI_BIAS_TANH_BF16 && TL::NW == 4 && TL::BN == 128) ? QKV2_W2_LDS : 0;
  __shared__ __attribute__((aligned(1024))) char lds[LDS_MAIN + LDS_W2];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / TL::WN, wn = wave % TL::WN;

  f32x16 acc[AI][AJ];
#pragma unroll
  for (int i = 0; i < AI; ++i)
#pragma unroll
    for (int j = 0; j < AJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
  if constexpr (SWAP && EPI == EPI_BIAS_TANH_BF16 && TL::NW == 4 && TL::BN == 128) {
    // fused Q/K/V stage 2: the accumulators start at bias / alpha, so the epilogue (short of
    // registers at 3 blocks per CU) holds no bias values
    if (P.qkv2_out) qkv2_stage_w2<TL>(P, lds + LDS_MAIN, n0, tid);  // read after the epilogue's barrier
    if ((P.qkv2_out || P.qkv2_h1_only) && P.bias) {  // (h1 only: the same h1 bits without stage 2)
      const float ia = 1.0f / P.alpha;
      const int hh = (tid & 63) >> 5;
#pragma unroll
      for (int i = 0; i < AI; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int n = n0 + wn * TL::TN * 32 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * hh;
          const float bv = n < N ? P.bias[n] * ia : 0.0f;
#pragma unroll
          for (int j = 0; j < AJ; ++j) acc[i][j][e] = bv;
        }
    }
  }

  if (ks0 < ks1) {
    const int lda = __builtin_amdgcn_readfirstlane(P.lda), ldb = __builtin_amdgcn_readfirstlane(P.ldb);
    // (the operand base pointers likewise: an MN-contiguous operand's descriptor is rebuilt per K-step)
    auto sgpr_ptr = [](const bf16_t* q) {
      const uint64_t v = (uint64_t)(uintptr_t)q;
      const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
      return (const bf16_t*)(uintptr_t)(((uint64_t)hi << 32) | lo);
    };
    const bf16_t* const Ap = sgpr_ptr(P.A);
    const bf16_t* const Bp = sgpr_ptr(P.B);
    // buffer descriptors (range-checked: OOB pieces read 0) from the tile's first row for a
    // K-contiguous operand; an MN-contiguous operand's descriptor is made per K-step (op_rsrc)
    const i32x4 ra_kc = A_KC ? op_rsrc<true>(Ap, lda, M, K, m0, 0) : i32x4{0, 0, 0, 0};
    const i32x4 rb_kc = B_KC ? op_rsrc<true>(Bp, ldb, N, K, n0, 0) : i32x4{0, 0, 0, 0};
    auto ra = [&](int k0) { return A_KC ? ra_kc : op_rsrc<false>(Ap, lda, M, K, m0, k0); };
    auto rb = [&](int k0) { return B_KC ? rb_kc : op_rsrc<false>(Bp, ldb, N, K, n0, k0); };
    const int nk = ks1 - ks0;
    // one K-step: stage U of the ring holds K-step tt (tt % ST == U), the step prefetches K-step
    // tt + ST - 1 into stage (U + ST - 1) % ST. U is a compile-time constant (the loop below is
    // unrolled by ST) so the LDS offsets of the DMA writes and of the fragment reads are static:
    // with a dynamic stage index hipcc cannot separate them and drains vmcnt(0) before the
    // fragment reads, serialising every K-step behind its own prefetch.
    auto step = [&](int tt, auto UC) {
      constexpr int U = decltype(UC)::value;
      // stage U landed for this wave: allow the younger stages' pieces to stay in flight
      wait_vm(PIECES * min(ST - 2, nk - 1 - tt));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave's pieces of stage U landed; the previous stage's reads done
      if (tt == 0) GEMM_STAMP(2);
      if (tt + ST - 1 < nk) {
        char* st = lds + ((U + ST - 1) % ST) * STAGE_BYTES;
        const int k0 = (ks0 + tt + ST - 1) * BK;
        issue_tile<BK, A_KC, GBM, NW>(ra(k0), st, lda, M, K, m0, k0, wave, lane);
        issue_tile<BK, B_KC, GBN, NW>(rb(k0), st + IMG_A, ldb, N, K, n0, k0, wave, lane);
      }
      const char* imgA = lds + U * STAGE_BYTES;
      const char* imgB = imgA + IMG_A;
#pragma unroll
      for (int s = 0; s < BK / 16; ++s) {
        bf16x8 fa[TM], fb[TN];
#pragma unroll
        for (int j = 0; j < TM; ++j) fa[j] = frag<BK, A_KC, GBM>(imgA, wm * TM * 32 + 32 * j, s, lane);
#pragma unroll
        for (int i = 0; i < TN; ++i) fb[i] = frag<BK, B_KC, GBN>(imgB, wn * TN * 32 + 32 * i, s, lane);
#pragma unroll
        for (int i = 0; i < AI; ++i)
#pragma unroll
          for (int j = 0; j < AJ; ++j) {
            if (SWAP) acc[i][j] = mfma32(fb[i], fa[j], acc[i][j]);
            else acc[i][j] = mfma32(fa[i], fb[j], acc[i][j]);
          }
      }
    };
#pragma unroll
    for (int t = 0; t < ST - 1; ++t)
      if (t < nk) {
        char* st = lds + t * STAGE_BYTES;
        const int k0 = (ks0 + t) * BK;
        issue_tile<BK, A_KC, GBM, NW>(ra(k0), st, lda, M, K, m0, k0, wave, lane);
        issue_tile<BK, B_KC, GBN, NW>(rb(k0), st + IMG_A, ldb, N, K, n0, k0, wave, lane);
      }
    GEMM_STAMP(1);
    int t = 0;
    for (; t + ST <= nk; t += ST) {
      step(t, std::integral_constant<int, 0>{});
      step(t + 1, std::integral_constant<int, 1>{});
      if constexpr (ST > 2) step(t + 2, std::integral_constant<int, (ST > 2 ? 2 : 0)>{});
      if constexpr (ST > 3) step(t + 3, std::integral_constant<int, (ST > 3 ? 3 : 0)>{});
    }
    if (t < nk) step(t, std::integral_constant<int, 0>{});
    if (ST > 2 && t + 1 < nk) step(t + 1, std::integral_constant<int, 1>{});
    if constexpr (ST > 3) { if (t + 2 < nk) step(t + 2, std::integral_constant<int, (ST > 3 ? 2 : 0)>{}); }
  }

  GEMM_STAMP(3);
  float alpha = P.alpha;
  if (P.alpha_ptr) alpha *= *P.alpha_ptr;
  // split-K into slabs: split s of the K loop writes its own fp32 slab (reduced by mmt_gemm_slab_reduce)
  float* o32 = P.o32 + (P.split_stride ? (int64_t)split * P.split_stride : (int64_t)0);
  const int h = lane >> 5, r = lane & 31;
  // the fused per-head Q/K/V stage 2 on the 128 x 128 tile only: next to the 256 x 256 tile's 128
  // accumulators it spills (the launcher refuses qkv2_out there; the engine then runs qkv2_fwd)
  if constexpr (SWAP && EPI == EPI_BIAS_TANH_BF16 && TL::NW == 4 && TL::BN == 128) {
    if (P.qkv2_out) {  // the per-head stage 2 of Q/K/V (uniform per problem)
      qkv2_fused<TL>(P, acc, lds, lds + LDS_MAIN, alpha, m0, n0, lane, wave);
      epilogue_swap<TL, EPI, EPI_ROWS, true>(P, acc, lds, o32, alpha, m0, n0, tid, lane, wave, det_of(batch, prob));
    } else if (P.qkv2_h1_only) {  // qkv2_fused's activation (the bias is in the accumulators), no stage 2
#pragma unroll
      for (int i = 0; i < AI; ++i)
#pragma unroll
        for (int j = 0; j < AJ; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = fast_tanh(alpha * acc[i][j][e]);
      epilogue_swap<TL, EPI, EPI_ROWS, true>(P, acc, lds, o32, alpha, m0, n0, tid, lane, wave, det_of(batch, prob));
    } else {
      epilogue_swap<TL, EPI, EPI_ROWS>(P, acc, lds, o32, alpha, m0, n0, tid, lane, wave, det_of(batch, prob));
    }
  } else if constexpr (SWAP) {
    epilogue_swap<TL, EPI, EPI_ROWS>(P, acc, lds, o32, alpha, m0, n0, tid, lane, wave, det_of(batch, prob));
  } else {
    // acc[i][j]: rows = m (sub-tile i), cols = n (sub-tile j)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * TN * 32 + 32 * j + r;
        if (n >= N) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = m0 + wm * TM * 32 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
          if (m < M) epi_scalar<EPI>(P, o32, alpha, m, n, acc[i][j][e]);
        }
      }
  }
  GEMM_STAMP(4);
}

// ---------------------------------------------------------------------------------------------
// MX-fp8 forward GEMM (C4's fp8 path): Y = X W^T with X [M][K], W [N][K] e4m3fn bytes and E8M0
// block exponents per 32 K elements, on v_mfma_scale_f32_32x32x64_f8f6f4 (2x the bf16 MFMA rate).
// Same structure as gemm_kernel (SWAP layout, LDS-DMA ring, XCD tile order, fused epilogues); a
// K-step is 128 fp8 = the 128-B image rows of the bf16 kernel's 64-element step, so the image
// geometry and swizzle are unchanged. Operand lane map (probed on gfx950: tools/probe/probe_mx.py):
// lane r + 32h of a 64-deep MFMA holds K elements [16h, 16h+16) and [32+16h, 48+16h) of row r in
// its 32 bytes, and its scale byte is the exponent of block h (K elements [32h, 32h+32)) of row r
// -> image chunks 4s + h and 4s + 2 + h, scale byte 2s + h of the row's K-step dword.
// ---------------------------------------------------------------------------------------------
template <int ROWS, int NW>
__device__ __forceinline__ void issue_tile_f8(const i32x4& rsrc, char* img, int ld, int rows_total, int K, int r0,
                                              int k0, int wave, int lane) {
  constexpr int PPW = ROWS * 128 / 1024 / NW;  // 1-KiB pieces per wave: 8 rows of 128 B
#pragma unroll
  for (int u = 0; u < PPW; ++u) {
    const int i = wave * PPW + u;
    const int row = 8 * i + lane / 8;
    const int chunk = kc_swz<64>(lane % 8, row);
    const int grow = r0 + row, gk = k0 + chunk * 16;
    const int voff = (grow < rows_total && gk < K) ? row * ld + gk : 0x7fffffff;  // rsrc from row r0
    dma16(rsrc, __builtin_amdgcn_readfirstlane(lds_u32(img + i * 1024)), voff);
  }
}

__device__ __forceinline__ i32x8 frag_f8(const char* img, int sb, int s, int lane) {
  const int row = sb + (lane & 31), h = lane >> 5;
  const u32x4 lo = *reinterpret_cast<const u32x4*>(img + row * 128 + kc_swz<64>(4 * s + h, row) * 16);
  const u32x4 hi = *reinterpret_cast<const u32x4*>(img + row * 128 + kc_swz<64>(4 * s + 2 + h, row) * 16);
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// one 4-B-per-lane LDS-DMA (buffer_load_dword ... lds): LDS[lds_addr + 4*lane] = buffer[voff]
__device__ __forceinline__ void dma4(const i32x4& rsrc, uint32_t lds_addr, int voff) {
  asm volatile("s_mov_b32 m0, %0\n\tbuffer_load_dword %1, %2, 0 offen lds"
               :
               : "s"(lds_addr), "v"(voff), "s"(rsrc)
               : "memory", "m0");
}

template <class TL, int EPI>
__global__ __launch_bounds__(TL::NT) void gemm_f8_kernel(GemmBatch batch) {
  constexpr int GBM = TL::BM, GBN = TL::BN, NW = TL::NW, NT = TL::NT, TM = TL::TM, TN = TL::TN;
  constexpr int ST = 2, KS = 128;                           // stages, K elements per step
  constexpr int IMG_A = GBM * 128, IMG_B = GBN * 128;       // e4m3 tiles
  constexpr int SC_A = GBM * 4, SC_B = GBN * 4;             // E8M0 dwords of the step, one per row
  constexpr int STAGE_BYTES = IMG_A + IMG_B + SC_A + SC_B;
  constexpr int SCDMA = (GBM + GBN) / 64;                   // dword LDS-DMAs of the exponents per stage
  static_assert(SCDMA <= NW, "one exponent DMA per wave at most");
  const GemmProblem& P = batch.p[blockIdx.z];
  const int M = P.M, N = P.N, K = P.K;
  const int tiles_n = (N + GBN - 1) / GBN, tiles_m = (M + GBM - 1) / GBM;
  int tile = blockIdx.x;
  {
    const int nwg = gridDim.x;
    const int x = tile % 8, q = nwg / 8, rr = nwg % 8;
    tile = (x < rr ? x * (q + 1) : rr * (q + 1) + (x - rr) * q) + tile / 8;
  }
  if (tile >= tiles_m * tiles_n) return;
  const int tm = tile / tiles_n, tn = tile % tiles_n;
  const int m0 = tm * GBM, n0 = tn * GBN;
  const int nk = (K + KS - 1) / KS;
  constexpr int EPI_ROWS = GBM == 128 ? 128 : 64;
  constexpr int RING = ST * STAGE_BYTES, CTILE = EPI_ROWS * (GBN + 4) * 4;
  __shared__ __attribute__((aligned(1024))) char lds[RING > CTILE ? RING : CTILE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / TL::WN, wn = wave % TL::WN;
  const int h = lane >> 5, r = lane & 31;
  f32x16 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
  // descriptors from the tile's first rows (32-bit offsets: see op_rsrc)
  const i32x4 ra = op_rsrc<true>(P.A, P.lda, M, K, m0, 0, 1);
  const i32x4 rb = op_rsrc<true>(P.B, P.ldb, N, K, n0, 0, 1);
  const i32x4 rsa = op_rsrc<true>(P.sa, P.lds_a, M, K, m0, 0, 1);
  const i32x4 rsb = op_rsrc<true>(P.sb, P.lds_b, N, K, n0, 0, 1);
  // the E8M0 dwords of a K-step ride the ring next to the tiles: wave w < SCDMA brings 64 rows' dwords
  // (rows past M / N land as zeros: exponent 2^-127 on zero-filled values)
  auto issue_scales = [&](char* st, int t) {
    if (wave >= SCDMA) return;
    const bool isa = wave < GBM / 64;
    const int row = (isa ? wave : wave - GBM / 64) * 64 + lane;
    const int grow = (isa ? m0 : n0) + row;
    const int voff = grow < (isa ? M : N) ? row * (isa ? P.lds_a : P.lds_b) + 4 * t : 0x7fffffff;
    char* dst = st + IMG_A + IMG_B + (isa ? 0 : SC_A) + (isa ? wave : wave - GBM / 64) * 256;
    dma4(isa ? rsa : rsb, __builtin_amdgcn_readfirstlane(lds_u32(dst)), voff);
  };
  issue_tile_f8<GBM, NW>(ra, lds, P.lda, M, K, m0, 0, wave, lane);
  issue_tile_f8<GBN, NW>(rb, lds + IMG_A, P.ldb, N, K, n0, 0, wave, lane);
  issue_scales(lds, 0);
  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // stage t landed for every wave; stage t-1's reads are done
    if (t + 1 < nk) {
      char* st = lds + ((t + 1) & 1) * STAGE_BYTES;
      issue_tile_f8<GBM, NW>(ra, st, P.lda, M, K, m0, (t + 1) * KS, wave, lane);
      issue_tile_f8<GBN, NW>(rb, st + IMG_A, P.ldb, N, K, n0, (t + 1) * KS, wave, lane);
      issue_scales(st, t + 1);
    }
    const char* imgA = lds + (t & 1) * STAGE_BYTES;
    const char* imgB = imgA + IMG_A;
    const uint32_t* scA = reinterpret_cast<const uint32_t*>(imgB + IMG_B);
    const uint32_t* scB = scA + GBM;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      // B fragments for the sub-step, A fragments one at a time (32-byte fragments)
      i32x8 fb[TN];
      uint32_t sb[TN];
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        fb[i] = frag_f8(imgB, wn * TN * 32 + 32 * i, s, lane);
        sb[i] = scB[wn * TN * 32 + 32 * i + r] >> (8 * (2 * s + h));
      }
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const i32x8 fa = frag_f8(imgA, wm * TM * 32 + 32 * j, s, lane);
        const uint32_t sa = scA[wm * TM * 32 + 32 * j + r] >> (8 * (2 * s + h));
#pragma unroll
        for (int i = 0; i < TN; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fb[i], fa, acc[i][j], 0, 0, 0, (int)sb[i], 0,
                                                                       (int)sa);
      }
    }
  }
  float alpha = P.alpha;
  if (P.alpha_ptr) alpha *= *P.alpha_ptr;
  epilogue_swap<TL, EPI, EPI_ROWS>(P, acc, lds, P.o32, alpha, m0, n0, tid, lane, wave);
}


// =============================================================================================
// Host half. One plan per launch (mmt_gemm_plan, mmt_gemm_plan.h) decides the kernel, its template
// arguments and the grid from the batch and the knobs below; the launchers launch what it says.
// =============================================================================================

// Every MMT_* environment variable of the GEMM launch policy and what its two setters write (DESIGN.md §3
// "GEMM knobs" has the same table), read once when the library loads. The measurement behind each default is
// beside the rule that uses it, in mmt_gemm_plan.
struct GemmKnobs {
  // mmt_gemm_set_variant (no variable): 128 x 128 pipeline of the forward / backward-data launches in bits 0-3
  // (-1: the per-epilogue policy) and of the atomic weight gradients in bits 4-7, 256 x 256 ring pipeline in bits
  // 8-11 (0: MMT_GEMM_BIG_VARIANT / default), bit 16 the 256 x 256 tile whatever K, bit 17 / 18 the ping-pong
  // kernel on everywhere it is built / off (-1: MMT_GEMM8 and its companions)
  int variant = -1, variant_dw = 0, big_variant_rt = 0, force_big = 0, gemm8_rt = -1;
  // MMT_GEMM_T2 / mmt_gemm_set_t2: 1 = every big launch with K below MMT_GEMM_BIG_KMIN on the 128 x 256 tile
  int t2 = mmt_env_int("MMT_GEMM_T2", 0);
  // MMT_GEMM_BIG=0: no 256 x 256 tile outside the row-wide launches
  int big = mmt_env_int("MMT_GEMM_BIG", 1);
  // MMT_GEMM_BIG_KMIN: K from which a launch whose problems all have M, N >= 256 takes the 256 x 256 tile
  int big_kmin = mmt_env_int("MMT_GEMM_BIG_KMIN", 1024);
  // MMT_GEMM_BIG_VARIANT: 256 x 256 ring pipeline of every launch (-1: BK 32 x 4 for the weight gradients, else 64 x 2)
  int big_variant = mmt_env_int("MMT_GEMM_BIG_VARIANT", -1);
  // MMT_GEMM8=0: the 256 x 256 ring instead of the ping-pong kernel everywhere
  int gemm8 = mmt_env_int("MMT_GEMM8", 1);
  // MMT_GEMM8_LN=0: only the row-wide (N = 256) LayerNorm-fused launches stay on the ring
  int gemm8_ln = mmt_env_int("MMT_GEMM8_LN", 1) != 0;
  // MMT_GEMM8_DW=1: the weight gradients on the ping-pong kernel too
  int gemm8_dw = mmt_env_int("MMT_GEMM8_DW", 0) != 0;
  // MMT_GEMM8_KMIN, MMT_GEMM8_MIN_TILES: a launch with K below MMT_GEMM_BIG_KMIN still goes big (on the ping-pong
  // kernel) from this K and this many 256 x 256 tiles on
  int gemm8_kmin = mmt_env_int("MMT_GEMM8_KMIN", 512);
  int gemm8_min_tiles = mmt_env_int("MMT_GEMM8_MIN_TILES", 1024);
  // MMT_GEMM_DW_VARIANT: 128 x 128 pipeline of the non-atomic launches with both operands MN-contiguous (-1: as the rest)
  int dw_variant = mmt_env_int("MMT_GEMM_DW_VARIANT", -1);
  // MMT_DW_SMALL=1: every weight gradient on the 128 x 128 tile (4x the tiles of the 256 x 256 one, so a quarter
  // of the K splits and of the split-K slab traffic at the ~128-block side-stream target)
  int dw_small = mmt_env_int("MMT_DW_SMALL", 0);
  // MMT_WGRAD_BLOCKS: blocks per weight-gradient launch the automatic split-K factor aims at (0: GemmBatch::dw_blocks / 128)
  int wgrad_blocks = mmt_env_int("MMT_WGRAD_BLOCKS", 0);
  // MMT_DW_XCD_PLANE=0: no XCD-major remap of the weight gradients' (tile, split, problem) grid
  int dw_xcd_plane = mmt_env_int("MMT_DW_XCD_PLANE", 1);
};
static GemmKnobs g_kn;

extern "C" int mmt_gemm_set_variant(int v) {
  if (v < 0) {  // back to the default policy
    g_kn.variant = -1; g_kn.variant_dw = 0; g_kn.big_variant_rt = 0; g_kn.force_big = 0; g_kn.gemm8_rt = -1;
    return 0;
  }
  if ((v & 15) > 6 || ((v >> 4) & 15) > 6 || ((v >> 8) & 15) > 3) return -1;
  g_kn.variant = v & 15;
  g_kn.variant_dw = (v >> 4) & 15;
  g_kn.big_variant_rt = (v >> 8) & 15;
  g_kn.force_big = (v >> 16) & 1;
  g_kn.gemm8_rt = ((v >> 17) & 1) ? 1 : ((v >> 18) & 1) ? 0 : -1;
  return 0;
}
extern "C" int mmt_gemm_set_t2(int v) {
  const int old = g_kn.t2;
  g_kn.t2 = v;
  return old;
}

// 128 x 256, 4 waves (TileL's per-wave 128 x 64) at two workgroups per CU (BK 32 x 3 stages: 72 KiB each), so one
// workgroup's prologue / epilogue overlaps the other's K loop
using TileM = TileCfg<1, 4, 4, 2>;
// ring depth of the 128 x 512 row-wide GEMMs (LayerNorm backward / forward fused): 3 stages of BK 32
// (120 KiB, one block per CU) against 2 (80 KiB, two blocks per CU): target step 20.39 -> 19.64 ms
// with the LayerNorm-backward GEMMs on it, 4 stages equal to 3 (profiles/r4k_ab.txt); at 2 stages the
// next K-step's DMA had one 32-deep step of MFMAs to hide under
#ifndef MMT_GEMM_W_ST
#define MMT_GEMM_W_ST 3
#endif
// default 128 x 128 pipelines (build-time, tools/build_variant.py A/B): bf16-output epilogues at 3
// blocks per CU (variant 6: BK 32 x 2), the others at 2 (variant 0: BK 64 x 2). Deeper rings lose
// in the step (round 4, profiles/r4m_ab.txt: variant 5 for the former C1 +0.6 %, variants 2 / 4 for
// the latter C1 +0.6 / +5.5 %, target +0.5 / +5.3 %)
#ifndef MMT_OCC3_VARIANT
#define MMT_OCC3_VARIANT 6
#endif
#ifndef MMT_DEF_VARIANT
#define MMT_DEF_VARIANT 0
#endif

// log2 of the tiles' rows and columns, by GemmTile (this runs before every launch: shifts, no divisions)
static constexpr int kTileShM[] = {7, 7, 8, 7}, kTileShN[] = {7, 8, 8, 9};
static_assert(TileS::BM == 1 << 7 && TileM::BM == 1 << 7 && TileL::BM == 1 << 8 && TileW::BM == 1 << 7, "kTileShM");
static_assert(TileS::BN == 1 << 7 && TileM::BN == 1 << 8 && TileL::BN == 1 << 8 && TileW::BN == 1 << 9, "kTileShN");

static int max_tiles(const GemmBatch& b, int tile, int* total) {
  const int shm = kTileShM[tile], shn = kTileShN[tile];
  int maxtiles = 0, sum = 0;
  for (int g = 0; g < b.count; ++g) {
    const GemmProblem& P = b.p[g];
    const int t = ((P.M + (1 << shm) - 1) >> shm) * ((P.N + (1 << shn) - 1) >> shn);
    maxtiles = t > maxtiles ? t : maxtiles;
    sum += t;
  }
  if (total) *total = sum;
  return maxtiles;
}
static int max_k(const GemmBatch& b) {
  int maxk = 0;
  for (int g = 0; g < b.count; ++g) maxk = std::max(maxk, b.p[g].K);
  return maxk;
}

// split-K factor of a weight-gradient launch (splits <= 0: automatic). Every split adds one fp32
// atomic per output element and an epilogue, so aim at ~2 blocks per CU for the 128x128 tile and
// ~1 for the 256x256 one, keeping >= 8 K-steps per split. Measured at C1 (128x128, grouped
// launches): 8 tiles 44.5 -> 29.2 us going from 8 to 32 splits, 24 tiles 50.7 -> 64.9 us from 8 to 22.
static int auto_splits(const GemmBatch& b, int tile, int splits) {
  if (splits > 0) return splits;
  int tiles = 0;
  max_tiles(b, tile, &tiles);
  if (tiles <= 0) return 1;
  // ~128 blocks: the weight gradients run on the side stream next to the data-gradient chain, so
  // half the chip for longer beats the whole chip with twice the split-K slab traffic (measured at
  // C1: 128 -> 9.97-10.28 ms/step, 256 -> 10.21-10.50, 64 -> 10.6)
  const int target = g_kn.wgrad_blocks > 0 ? g_kn.wgrad_blocks : b.dw_blocks > 0 ? b.dw_blocks : 128;
  const int maxs = std::max(1, std::min(32, max_k(b) / 512));
  return std::max(1, std::min(target / tiles, maxs));
}

static bool has_qkv2(const GemmBatch& b) {
  for (int g = 0; g < b.count; ++g)
    if (b.p[g].qkv2_out || b.p[g].qkv2_h1_only) return true;
  return false;
}

// variant bit 17 / 18 force the ping-pong kernel on / off (the kernel tests)
static bool gemm8_on() {
  // default on (round 5): C4 355 -> 350 ms/step, C3 153.3 -> 152.4, target / C1 neutral (same-box A/B,
  // profiles/r5_gemm8_mlp2_ab.txt); MMT_GEMM8=0 restores the 2-stage 256 x 256 ring everywhere
  return g_kn.gemm8_rt >= 0 ? g_kn.gemm8_rt != 0 : g_kn.gemm8 != 0;
}

// tile policy: the 256x256 tile where every problem of the launch fills it (M, N >= 256) and the
// K loop is long enough to amortise its prologue/epilogue (K >= MMT_GEMM_BIG_KMIN; weight gradients
// always qualify: K = B*T). MMT_GEMM_BIG=0 disables it.
// K threshold 1024 (round 2 c): at K = 512 (d512 forward GEMMs and data gradients) the 128x128 tile at
// 2-3 blocks per CU overlaps one block's epilogue with the others' K loops and shares the chip with
// the side stream better than the single 256x256 block per CU (target step 23.13 -> 22.73 ms)
// Shorter K on the ping-pong kernel for launches with many tiles: at K = 512 it wins where
// the launch has >= 4 tiles per CU (the target's ffn0 and ffn2 dX: 221 -> 177 and 252 -> 230 us
// standalone; smaller launches leave CUs idle or lose the 128 x 128 tile's 2-3 blocks per CU beside the
// side stream: every K = 512 launch on it measured +1 % on the target step)
static bool use_big(const GemmBatch& b) {
  if (!g_kn.big || b.count == 0) return false;
  bool big = true;
  int tiles = 0;
  for (int g = 0; g < b.count; ++g) {
    const GemmProblem& P = b.p[g];
    if (P.M < TileL::BM || P.N < TileL::BN) return false;
    if (P.K < g_kn.big_kmin && !g_kn.force_big) big = false;
    tiles += ((P.M + 255) / 256) * ((P.N + 255) / 256);
  }
  if (big) return true;
  // shorter K on the ping-pong kernel: only big launches, and never the fused Q/K/V stage 2 (128 x 128 only)
  if (!gemm8_on() || has_qkv2(b) || tiles < g_kn.gemm8_min_tiles) return false;
  for (int g = 0; g < b.count; ++g)
    if (b.p[g].K < g_kn.gemm8_kmin) return false;
  return true;
}

// 16-byte LDS-DMA pieces need 8-element-aligned leading dimensions (mask 7; fp8 bytes: 15) and 16-byte aligned bases
static bool operands_ok(const GemmProblem& P, int ldmask) {
  return !((P.lda | P.ldb) & ldmask) && !(((uintptr_t)P.A | (uintptr_t)P.B) & 15);
}

// the fused per-head Q/K/V stage 2 (qkv2_fused): forward tanh epilogue only, hh 16 or 32, 16-B stores,
// whole hh-blocks (N % hh == 0)
static bool qkv2_ok(const GemmProblem& P, int epi, bool fwd) {
  // (h1 only: the fused launch's accumulator start and activation without stage 2, same kernel)
  if (!P.qkv2_out) return !P.qkv2_h1_only || (epi == EPI_BIAS_TANH_BF16 && fwd && !P.alpha_ptr && P.alpha != 0.0f);
  // (no alpha_ptr, alpha != 0: the accumulators start at bias / alpha)
  return epi == EPI_BIAS_TANH_BF16 && fwd && (P.qkv2_hh == 16 || P.qkv2_hh == 32) && P.N % P.qkv2_hh == 0 &&
         !P.alpha_ptr && P.alpha != 0.0f &&
         P.qkv2_w2 && !(P.qkv2_ld & 7) && !((uintptr_t)P.qkv2_out & 15) && !((uintptr_t)P.qkv2_w2 & 15);
}

// tile-local operand spans (op_rsrc) must stay below 2^31 bytes: at most 512 rows (or a 64-deep K-step)
// of the leading dimension plus K (weight-gradient slabs and outputs use 64-bit offsets)
static bool gemm_span_ok(const GemmBatch& b) {
  for (int g = 0; g < b.count; ++g) {
    const GemmProblem& P = b.p[g];
    if (P.M < 0 || P.N < 0 || P.K < 0 || P.lda < 0 || P.ldb < 0) return false;
    if ((int64_t)(512 + 1) * std::max(P.lda, P.ldb) * 2 + (int64_t)P.K * 2 >= ((int64_t)1 << 31)) return false;
  }
  return true;
}

// the row-wide launches (a tile as wide as the row: its block owns whole rows of the LayerNorm): every problem
// N == 256 or N == 512, all alike, 16-B aligned rows; ln_bwd: EPI_LN_BWD_F32's operands, else the forward's lnf_*
static bool row_wide_ok(const GemmBatch& b, bool ln_bwd) {
  if (b.count == 0) return false;
  for (int g = 0; g < b.count; ++g) {
    const GemmProblem& P = b.p[g];
    if ((P.N != TileL::BN && P.N != TileW::BN) || P.N != b.p[0].N || !P.resid || !P.o32 || (P.ldc & 3) ||
        (P.ldres & 3) || (P.o16 && (P.ldo16 & 7)) || !operands_ok(P, 7) || (((uintptr_t)P.o32 | (uintptr_t)P.resid) & 15))
      return false;
    if (ln_bwd) {  // (o16: the epilogue's 16-B dropout-masked copy stores)
      if (!P.ln_gamma || !P.ln_mean || !P.ln_rstd || !P.ln_dgamma || !P.ln_dbeta ||
          (((uintptr_t)P.ln_gamma | (uintptr_t)P.o16) & 15))
        return false;
    } else if (P.lnf_y && (!P.lnf_gamma || !P.lnf_beta || !P.lnf_mean || !P.lnf_rstd ||
                           (((uintptr_t)P.lnf_y | (uintptr_t)P.lnf_gamma | (uintptr_t)P.lnf_beta) & 15))) {
      return false;
    }
  }
  return true;
}
bool mmt_gemm_resid_ln_ok(const GemmBatch& b) { return row_wide_ok(b, false); }
bool mmt_gemm_ln_bwd_ok(const GemmBatch& b) { return row_wide_ok(b, true); }

static bool f8_ok(const GemmProblem& P) {
  if ((P.K & 31) || !operands_ok(P, 15) || (P.lds_a & 3) || (P.lds_b & 3) ||
      (((uintptr_t)P.sa | (uintptr_t)P.sb) & 3) || P.lds_a * 32 < P.K || P.lds_b * 32 < P.K)
    return false;
  if (P.o8 && ((P.N & 31) || (P.ld8 & 7) || ((uintptr_t)P.o8 & 7))) return false;
  return !P.qkv2_out && !P.qkv2_h1_only;  // (no fused Q/K/V stage 2 on the fp8 kernel)
}

// slab elements of one weight-gradient split over all problems (each problem's slab 16-B aligned)
static int64_t slab_elems(const GemmBatch& b) {
  int64_t per = 0;
  for (int g = 0; g < b.count; ++g) per += ((int64_t)b.p[g].M * b.p[g].N + 3) / 4 * 4;
  return per;
}

GemmPlan mmt_gemm_plan(const GemmBatch& b, int kind, bool a_kc, bool b_kc, int epi, int splits, int64_t slab_bytes) {
  const GemmKnobs& kn = g_kn;
  const bool linear = kind == GEMM_LINEAR, wgrad = kind == GEMM_WGRAD, f8 = kind == GEMM_F8;
  const bool row_wide = kind == GEMM_RESID_LN || kind == GEMM_LN_BWD;
  GemmPlan p{};
  p.status = GEMM_PLAN_INVALID;
  p.minb = 1;
  p.swap = 1;
  // the kernel's operand layouts and epilogue; (layouts, epilogue) outside the family's list: invalid
  gemm_kind_ops(kind, a_kc, b_kc, epi);
  p.a_kc = a_kc; p.b_kc = b_kc; p.epi = epi;
  if (b.count == 0 && (wgrad || f8)) { p.status = GEMM_PLAN_EMPTY; return p; }
  bool built = row_wide || wgrad;
  if (linear) {
    switch (gemm_op_key(a_kc, b_kc, epi)) {
#define X(A, B, SW, E) case gemm_op_key(A, B, E): built = true; p.swap = SW; break;
      GEMM_RING_OPS(X)
#undef X
    }
  } else if (f8) {
    switch (epi) {
#define X(E) case E:
      GEMM_F8_OPS(X) built = true;
#undef X
    }
  }
  if (!built) return p;
  if (b.count == 0 && linear) { p.status = GEMM_PLAN_EMPTY; return p; }

  // ---- tile -------------------------------------------------------------------------------------------
  bool big;
  if (f8) {
    // the 256x256 tile where every problem fills it and K is long (as the bf16 policy), else 128x128 (tile_hint 1:
    // the 128 x 128 tile, which fits beside other streams' waves where the 256 x 256 one needs a free CU)
    big = kn.big != 0 && b.tile_hint != 1;
    for (int g = 0; g < b.count; ++g)
      if (b.p[g].M < TileL::BM || b.p[g].N < TileL::BN || b.p[g].K < kn.big_kmin) big = false;
  } else {
    // MMT_DW_SMALL / GemmBatch::tile_hint 2: this weight gradient on the 128 x 128 tile, 64 KiB of LDS, which fits on a
    // CU beside the main stream's 80 KiB attention-backward workgroups where the 256 x 256 one's 128 KiB does not
    big = use_big(b) && !(wgrad && (kn.dw_small || b.tile_hint == 2));
  }
  p.tile = big ? GEMM_TILE_256 : GEMM_TILE_128;
  // row-wide, whatever K: 256 x 256 at C = 256, 128 x 512 at C = 512 (BK 64 measured neutral there, a
  // 128 x 256 tile at C = 256 slower: 63.7 -> 92.9 us per launch, profiles/r3i_lnb_tile_ab.txt)
  if (row_wide) p.tile = b.p[0].N == TileW::BN ? GEMM_TILE_128x512 : GEMM_TILE_256;
  if (wgrad) {  // the split-K factor, capped by the slab's capacity; without a slab one K pass
    splits = auto_splits(b, p.tile, 0);
    const int64_t cap = slab_bytes > 0 ? slab_bytes / (int64_t)sizeof(float) / std::max<int64_t>(1, slab_elems(b)) : 1;
    if (splits > cap) splits = (int)cap;
    p.slabs = splits > 1;  // (one K pass accumulates straight into the gradient)
    p.epi = epi = p.slabs ? EPI_STORE_F32 : EPI_ACC_F32;
    p.xcd_plane = kn.dw_xcd_plane;
    int64_t maxn4 = 0;
    for (int g = 0; g < b.count; ++g) maxn4 = std::max<int64_t>(maxn4, ((int64_t)b.p[g].M * b.p[g].N + 3) / 4);
    p.reduce_blocks = p.slabs ? (int)std::min<int64_t>(4096, (maxn4 + 255) / 256) : 0;
  }
  // MMT_GEMM_T2=1 / tile_hint 1: the big launches with K below the 256 x 256 tile's threshold (K = 512: the d512
  // FFN and cross-attention K/V products the ping-pong kernel takes by default) on the 128 x 256 tile (SWAP
  // non-atomic epilogues only)
  if ((linear || wgrad) && big && p.swap && epi != EPI_ATOMIC_F32 && (kn.t2 || b.tile_hint == 1) && max_k(b) < kn.big_kmin)
    p.tile = GEMM_TILE_128x256;

  // ---- validity -----------------------------------------------------------------------------------------
  if (!gemm_span_ok(b)) return p;
  if (row_wide && !row_wide_ok(b, kind == GEMM_LN_BWD)) return p;
  for (int g = 0; g < b.count; ++g) {
    const GemmProblem& P = b.p[g];
    if (f8 ? !f8_ok(P) : !operands_ok(P, 7)) return p;
    if (linear && !qkv2_ok(P, epi, a_kc && b_kc)) return p;
  }
  if (linear && big && has_qkv2(b)) return p;  // fused stage 2: 128 x 128 tile only

  // ---- grid ---------------------------------------------------------------------------------------------
  p.gx = max_tiles(b, p.tile, nullptr);
  p.gz = b.count;
  const bool split_k = wgrad || epi == EPI_ATOMIC_F32 || (!a_kc && !b_kc && epi == EPI_STORE_F32);
  p.gy = epi == EPI_ATOMIC_F32 ? auto_splits(b, p.tile, splits) : split_k ? std::max(1, splits) : 1;
  if (p.gx == 0) { p.status = GEMM_PLAN_EMPTY; return p; }
  p.status = GEMM_PLAN_OK;

  // ---- kernel family and pipeline -------------------------------------------------------------------------
  p.family = GEMM_RING; p.bk = 64; p.stages = 2;
  if (f8) {
    p.family = GEMM_FP8; p.bk = 128;
  } else if (p.tile == GEMM_TILE_128x512) {
    p.bk = 32; p.stages = MMT_GEMM_W_ST;
  } else if (p.tile == GEMM_TILE_128x256) {
    p.bk = 32; p.stages = 3; p.minb = 2;
  } else if (p.tile == GEMM_TILE_256) {
    // forward / backward-data products on the ping-pong kernel; the weight gradients (both operands
    // MN-contiguous) only with MMT_GEMM8_DW=1: standalone 2-4 % faster, but on the side stream beside the
    // main stream's attention backward the step measured slower (C1 attention backward 198 -> 207 us live,
    // the *_dw family 107 -> 113 us; profiles/r5_gemm8_mlp2_ab.txt). The row-wide tile takes it too (same
    // epilogue, LayerNorm included) unless MMT_GEMM8_LN=0; variant bit 17 forces it everywhere.
    const bool on8 = row_wide ? (kn.gemm8_rt >= 0 ? kn.gemm8_rt == 1 : gemm8_on() && kn.gemm8_ln)
                              : gemm8_on() && (a_kc || kn.gemm8_dw || kn.gemm8_rt == 1);
    if (on8 && p.swap && gemm8_supports(a_kc, b_kc, epi)) {
      p.family = GEMM_PINGPONG;
    } else if (!row_wide) {
      // 256x256 ring pipeline: 0 = BK 64 x 2 stages, 1 = BK 32 x 4 (three K-steps in flight), 2 = BK 32 x 3,
      // 3 = BK 32 x 2 (66.5 KiB with the epilogue tile: leaves room on its CU for an 80 KiB attention-backward
      // workgroup beside it; measured for the weight gradients). Round 4 also built a
      // software-pipelined K-step (the next sub-step's fragments read while this one's MFMAs issue, the prefetch
      // pieces spread between MFMAs) and a persistent 256 x 256 kernel that prefetches the next tile's first stage
      // under the last K-step and the epilogue. Both won standalone (tools/gemm_bench.py: 4096^3 1136 -> 1180
      // TF/s, C4 ffn0 889 -> 915) and lost in the training step beside the side stream (C1 8.78 -> 8.88 ms/step,
      // target 20.47 -> 20.98), so they were removed at the end of round 4.
      // Default: BK 32 x 4 for the weight gradients (both operands MN-contiguous, K = B*T: 128+ K-steps, the
      // deeper ring keeps three in flight; C1 *_dw family 3.44 -> 3.20 ms/step live, C3 73.8 -> 69.4),
      // BK 64 x 2 for the rest (the forward / data-gradient 256 x 256 launches measured 0.3-0.9 % slower
      // at BK 32 x 4 in C3 / C4: profiles/r4z_big_variant_ab.txt). MMT_GEMM_BIG_VARIANT sets all of them.
      const int bv = kn.big_variant_rt ? kn.big_variant_rt : kn.big_variant >= 0 ? kn.big_variant : (!a_kc && !b_kc) ? 1 : 0;
      if (bv >= 1 && bv <= 3) { p.bk = 32; p.stages = 5 - bv; }
    }
  } else {
    // default policy (variant knob unset): bf16-output epilogues with no aux operand stage 64 rows
    // per epilogue pass and run 3+ blocks per CU (variant 6: 33 KB of LDS instead of 66 KB), which
    // overlaps one block's short K loop with the others' prologue / stores; epilogues that read an aux
    // or residual operand or store fp32 measured faster at 2 blocks per CU with the 64-deep ring
    // (profiles/r2_gemm_bench.txt)
    // (a 256 x 128 tile at two blocks per CU won standalone on the target ffn0, 214 -> 194 us, but not in
    // the step beside the side stream, 20.21 -> 20.37 ms: profiles/r3y_tilem_ab.txt; removed in round 4)
    // (the ReLU' epilogue reading bits has no 16-B aux operand left, but at 3 blocks per CU it measured
    // neutral: C1 8.558 vs 8.555, target 19.937 vs 19.935 ms, profiles/r5ac_drelu_occ3_ab.txt)
    const bool occ3 = epi == EPI_STORE_BF16 || epi == EPI_BIAS_TANH_BF16 || epi == EPI_BIAS_RELU_BF16;
    const int var = epi == EPI_ATOMIC_F32                      ? kn.variant_dw
                    : (!a_kc && !b_kc && kn.dw_variant >= 0) ? kn.dw_variant
                    : kn.variant >= 0                          ? kn.variant
                    : occ3                                     ? MMT_OCC3_VARIANT
                                                               : MMT_DEF_VARIANT;
    // 0 = BK 64 x 2 stages, 1 = BK 32 x 2, 2 = BK 32 x 3, 3 = BK 32 x 4, 4 = BK 64 x 3,
    // 5 = BK 32 x 3 and 6 = BK 32 x 2 at 3 blocks per CU (64-row epilogue passes)
    static constexpr int kVar[7][3] = {{64, 2, 1}, {32, 2, 1}, {32, 3, 1}, {32, 4, 1}, {64, 3, 1}, {32, 3, 3}, {32, 2, 3}};
    if (var >= 1 && var <= 6) { p.bk = kVar[var][0]; p.stages = kVar[var][1]; p.minb = kVar[var][2]; }
  }
  return p;
}

// ---- plan -> template instantiation, once per kernel family -------------------------------------------------
template <class TL, int BK, int ST, bool A_KC, bool B_KC, bool SWAP, int EPI, int MINB = 1>
static hipError_t launch_v(const GemmBatch& b, const GemmPlan& p, hipStream_t s) {
  const dim3 grid(p.gx, p.gy, p.gz);
#ifdef MMT_GEMM_STAMPS
  GemmBatch bs = b;
  bs.stamps = g_stamps;
  hipLaunchKernelGGL((gemm_kernel<TL, BK, ST, A_KC, B_KC, SWAP, EPI, MINB>), grid, dim3(TL::NT), 0, s, bs);
#else
  hipLaunchKernelGGL((gemm_kernel<TL, BK, ST, A_KC, B_KC, SWAP, EPI, MINB>), grid, dim3(TL::NT), 0, s, b);
#endif
  return hipGetLastError();
}

constexpr int ring_key(int tile, int bk, int stages, int minb) { return (tile << 16) | (bk << 8) | (stages << 4) | minb; }
// the ring: 128 x 128 in seven pipelines and 256 x 256 in four for every GEMM_RING_OPS entry, 128 x 256 for its SWAP
// non-atomic ones, 128 x 512 for the two row-wide epilogues; LayerNorm backward only on the two row-wide tiles
template <bool A_KC, bool B_KC, bool SWAP, int EPI>
static hipError_t launch_ring(const GemmBatch& b, const GemmPlan& p, hipStream_t s) {
  constexpr bool ln_bwd = EPI == EPI_LN_BWD_F32;
  constexpr bool row_wide = ln_bwd || (A_KC && B_KC && EPI == EPI_BIAS_RESID_F32);
  const int v = ring_key(p.tile, p.bk, p.stages, p.minb);
#define V(TL, TILE, BK, ST, MINB) \
  if (v == ring_key(TILE, BK, ST, MINB)) return launch_v<TL, BK, ST, A_KC, B_KC, SWAP, EPI, MINB>(b, p, s);
  if constexpr (!ln_bwd) { V(TileS, GEMM_TILE_128, 32, 2, 3) V(TileS, GEMM_TILE_128, 64, 2, 1) }  // (the defaults first)
  V(TileL, GEMM_TILE_256, 64, 2, 1)
  if constexpr (row_wide) V(TileW, GEMM_TILE_128x512, 32, MMT_GEMM_W_ST, 1)
  if constexpr (!ln_bwd) {
    V(TileL, GEMM_TILE_256, 32, 4, 1) V(TileL, GEMM_TILE_256, 32, 3, 1) V(TileL, GEMM_TILE_256, 32, 2, 1)
    V(TileS, GEMM_TILE_128, 32, 2, 1) V(TileS, GEMM_TILE_128, 32, 3, 1) V(TileS, GEMM_TILE_128, 32, 4, 1)
    V(TileS, GEMM_TILE_128, 64, 3, 1) V(TileS, GEMM_TILE_128, 32, 3, 3)
    if constexpr (SWAP && EPI != EPI_ATOMIC_F32) V(TileM, GEMM_TILE_128x256, 32, 3, 2)
  }
#undef V
  return hipErrorInvalidValue;
}

static hipError_t launch_plan(const GemmBatch& b, const GemmPlan& p, hipStream_t s) {
  if (p.status != GEMM_PLAN_OK) return p.status == GEMM_PLAN_EMPTY ? hipSuccess : hipErrorInvalidValue;
  if (p.family == GEMM_PINGPONG) return mmt_launch_gemm8(b, p, s);
  if (p.family == GEMM_FP8) {
    switch (p.epi) {
#define X(E)                                                                                                      \
  case E:                                                                                                         \
    if (p.tile == GEMM_TILE_256) hipLaunchKernelGGL((gemm_f8_kernel<TileL, E>), dim3(p.gx, p.gy, p.gz), dim3(TileL::NT), 0, s, b); \
    else hipLaunchKernelGGL((gemm_f8_kernel<TileS, E>), dim3(p.gx, p.gy, p.gz), dim3(TileS::NT), 0, s, b);         \
    return hipGetLastError();
      GEMM_F8_OPS(X)
#undef X
    }
    return hipErrorInvalidValue;
  }
  switch (gemm_op_key(p.a_kc, p.b_kc, p.epi)) {
#define X(A, B, SW, E) case gemm_op_key(A, B, E): return launch_ring<A, B, SW, E>(b, p, s);
    GEMM_RING_OPS(X) GEMM_RING_LN_BWD_OP(X)
#undef X
  }
  return hipErrorInvalidValue;
}

// Deterministic mode (GemmBatch::det, mmt_det.h): the epilogue's column sums (dbias; with `ln` also
// ln_dgamma / ln_dbeta) are stored per row tile at [slot][ceil(M / 128)][N] of the problem's scratch and
// one ordered sum behind the launch adds them into the gradients
static int64_t gemm_det_stride(const GemmBatch& b, bool ln) {
  int64_t st = 0;
  for (int g = 0; g < b.count; ++g) {
    const int64_t nrt = (b.p[g].M + MMT_DET_GEMM_ROWS - 1) / MMT_DET_GEMM_ROWS;
    st = std::max(st, (ln ? 3 : 1) * nrt * (int64_t)b.p[g].N);
  }
  return (st + 3) & ~(int64_t)3;
}
int64_t mmt_gemm_det_floats(int count, int M, int N, bool ln) {
  GemmBatch b{};
  b.count = 1; b.p[0].M = M; b.p[0].N = N;
  return count * gemm_det_stride(b, ln);
}
template <class F>
static hipError_t gemm_det_run(const GemmBatch& b, bool ln, hipStream_t s, F run) {
  if (!b.det.base) return run(b);
  bool any = false;
  for (int g = 0; g < b.count; ++g) any = any || b.p[g].dbias || (ln && (b.p[g].ln_dgamma || b.p[g].ln_dbeta));
  GemmBatch d = b;
  if (!any) {  // no column sums leave this launch
    d.det = DetScratch{};
    return run(d);
  }
  d.det.stride = gemm_det_stride(b, ln);
  DetLaunch L;
  hipError_t e = L.begin(d.det, b.count, d.det.stride, s);
  if (e != hipSuccess) return e;
  e = run(d);
  if (e != hipSuccess) return e;
  for (int g = 0; g < b.count; ++g) {
    const GemmProblem& P = b.p[g];
    const int nrt = (P.M + MMT_DET_GEMM_ROWS - 1) / MMT_DET_GEMM_ROWS;
    const int64_t slot = (int64_t)nrt * P.N;
    L.seg(g, d.det.stride, 0, P.dbias, nrt, P.N);
    if (ln) {
      L.seg(g, d.det.stride, slot, P.ln_dgamma, nrt, P.N);
      L.seg(g, d.det.stride, 2 * slot, P.ln_dbeta, nrt, P.N);
    }
  }
  return L.finish();
}

hipError_t mmt_launch_gemm(const GemmBatch& b, bool a_kc, bool b_kc, int epi, int splits, hipStream_t s) {
  return gemm_det_run(b, false, s, [&](const GemmBatch& d) {
    return launch_plan(d, mmt_gemm_plan(d, GEMM_LINEAR, a_kc, b_kc, epi, splits, 0), s);
  });
}
hipError_t mmt_launch_gemm_ln_bwd(const GemmBatch& b, hipStream_t s) {
  return gemm_det_run(b, true, s, [&](const GemmBatch& d) {
    return launch_plan(d, mmt_gemm_plan(d, GEMM_LN_BWD), s);
  });
}
hipError_t mmt_launch_gemm_resid_ln(const GemmBatch& b, hipStream_t s) {
  return launch_plan(b, mmt_gemm_plan(b, GEMM_RESID_LN), s);
}
hipError_t mmt_launch_gemm_f8(const GemmBatch& b, int epi, hipStream_t s) {
  return launch_plan(b, mmt_gemm_plan(b, GEMM_F8, true, true, epi, 1, 0), s);
}

// ---------------------------------------------------------------------------------------------
// Weight gradients dW[M, N] += alpha * dY[K, M]^T X[K, N] (both operands MN-contiguous, K = rows).
// K = B*T is long and M x N small, so the K loop is split over workgroups. Each split writes a
// plain fp32 slab (row-coalesced 16-B stores of the staged epilogue) and one reduce pass adds the
// slabs into the gradient. Measured alternatives (C1, same box): per-element fp32
// atomics (16.7 M per FFN launch, ~60 of its ~85 us), and three in-kernel reductions with no
// reduce launch (pairwise tree, every-split slice combine behind a per-tile arrival barrier, last
// arriver) were all slower than this: the reduce launch runs on the side stream beside the
// data-gradient chain, while an in-kernel reduction holds CUs waiting or reading serially.
// ---------------------------------------------------------------------------------------------
struct SlabProblem {
  const float* slab;  // [splits][M * N]
  float* out;         // [M][ldc]
  int M, N, ldc;
  int64_t stride;     // elements per slab
};
struct SlabBatch {
  SlabProblem p[MMT_MAX_GROUP];
  int count, splits;
};

__global__ __launch_bounds__(256) void slab_reduce_kernel(SlabBatch b) {
  const SlabProblem& P = b.p[blockIdx.y];
  const bool vec = (P.N % 4 == 0) && (P.ldc % 4 == 0) && (((uintptr_t)P.out & 15) == 0);
  // kernel arguments the split loop reads, as values (read through P they were re-loaded per split group)
  const int splits = __builtin_amdgcn_readfirstlane(b.splits);
  const int64_t stride = P.stride;
  const float* const slab = P.slab;
  if (vec) {
    const int64_t n4 = (int64_t)P.M * P.N / 4;
    const int N4 = P.N / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      // 8 slab loads in flight per thread (independent partial sums)
      f32x4 part[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) part[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      int sp = 0;
      for (; sp + 8 <= splits; sp += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) part[u] += reinterpret_cast<const f32x4*>(slab + (sp + u) * stride)[i];
      }
      for (; sp < splits; ++sp) part[0] += reinterpret_cast<const f32x4*>(slab + sp * stride)[i];
      const f32x4 acc = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
      const int m = (int)(i / N4), c = (int)(i % N4) * 4;
      float* o = P.out + (int64_t)m * P.ldc + c;
      *reinterpret_cast<f32x4*>(o) = *reinterpret_cast<const f32x4*>(o) + acc;
    }
  } else {
    const int64_t n = (int64_t)P.M * P.N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
      float acc = P.slab[i];
      for (int sp = 1; sp < b.splits; ++sp) acc += P.slab[sp * P.stride + i];
      P.out[(int64_t)(i / P.N) * P.ldc + i % P.N] += acc;
    }
  }
}

hipError_t mmt_launch_gemm_wgrad(const GemmBatch& b, float* slab, int64_t slab_bytes, hipStream_t s) {
  const GemmPlan p = mmt_gemm_plan(b, GEMM_WGRAD, false, false, 0, 0, slab ? slab_bytes : 0);
  GemmBatch d = b;
  d.xcd_plane = p.xcd_plane;
  SlabBatch sb{};
  sb.count = b.count;
  sb.splits = p.gy;
  const int64_t per = p.slabs ? slab_elems(b) : 0;
  int64_t off = 0;
  for (int g = 0; g < d.count; ++g) {
    GemmProblem& P = d.p[g];
    P.split_stride = per;
    if (!p.slabs) continue;  // one K pass: accumulate straight into the gradient
    sb.p[g] = SlabProblem{slab + off, P.o32, P.M, P.N, P.ldc, per};
    P.o32 = slab + off;
    P.ldc = P.N;
    off += ((int64_t)P.M * P.N + 3) / 4 * 4;
  }
  const hipError_t e = launch_plan(d, p, s);
  // (a batch without tiles has one split, so an EMPTY plan never has slabs to reduce)
  if (e != hipSuccess || !p.slabs || p.status != GEMM_PLAN_OK) return e;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(p.reduce_blocks, p.gz), dim3(256), 0, s, sb);
  return hipGetLastError();
}
