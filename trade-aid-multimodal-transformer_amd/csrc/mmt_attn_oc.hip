// Causal self-attention forward at hs 32 with Q / K / V made on chip (AttnProblem::oc_*; the rest of the attention
// kernels: mmt_attn.hip). A translation unit of its own: with this kernel in mmt_attn.hip, hipcc allocated
// attn_fwd_kernel<32, true> (the cross-attention's and the eval forward's kernel, whose text did not change) 171
// VGPRs instead of 167, past the 168 that three waves per SIMD allow.
#include "mmt_attn_dev.h"
#include "mmt_attn_plan.h"

// =============================================================================================
// forward at hs 32, T <= 256, one KV stream, with Q / K / V made on chip (AttnProblem::oc_*): grid (B*H, 1, G),
// one workgroup per (batch, head), the walk and the output epilogue of attn_fwd_kernel<32> with its one chunk.
// No Q / K / V rows are read: wave w makes the K, V and Q rows of its own two tiles (w and 7 - w: between them
// the waves cover all eight) from h1 and W2, one MFMA per tile and kind (oc_tile). The K / V pieces go to ks /
// vs, the Q pieces are the qf fragments as they are; rows >= T read h1 as zeros, so their K / V / Q are zero as
// the staged rows of attn_fwd_kernel are.
// =============================================================================================
template <bool DROP>
__global__ __launch_bounds__(256, MMT_FWD_MINB(32)) void attn_fwd_oc32_kernel(AttnBatch batch, int T, int H, float scale) {
  constexpr int HS = 32;
  using G = Geo<HS>;
  constexpr int ROWS = Chunk<HS>::ROWS;
  constexpr int MKT = ROWS / 32;     // key tiles of the chunk
  constexpr int MDW = 8 * MKT * 32;  // keep-bit dwords
  const AttnProblem& P = batch.p[blockIdx.z];
  const int bh = xcd_tile(blockIdx.x, gridDim.x), b = bh / H, head = bh % H;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int nt = (T + 31) / 32;
  const int64_t rowbase = (int64_t)b * T;
  const float c2 = scale * kLog2e;
  __shared__ __attribute__((aligned(16))) bf16_t ks[ROWS * G::RW];
  __shared__ __attribute__((aligned(16))) bf16_t vs[ROWS * G::TW];
  using MS = MaskStager<HS>;
  __shared__ __attribute__((aligned(16))) uint32_t msk[DROP ? MDW : 4];  // keep-bit lane words
  const int64_t lw_off = (int64_t)gridDim.x * (nt * (nt + 1) / 2) * 32;   // lane-word record: after the key-major one
  MS mst;
  const int qa = w, qb = 7 - w;           // qa < qb
  const bool la = qa < nt, lb = qb < nt;  // lb implies la
  FwdQ<HS> A, Bq;
  A.tq = qa * 32 + r;
  Bq.tq = qb * 32 + r;
  {
    bf16x8 wf[3], hf[2][3];
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) {
      const int blk = kd * H + head;
      wf[kd] = oc_w2frag(P.oc_w2, blk, r, h);
      hf[0][kd] = oc_hfrag(P.oc_h1 + (rowbase + A.tq) * P.oc_ld + blk * 16, h, A.tq < T);
      hf[1][kd] = oc_hfrag(P.oc_h1 + (rowbase + Bq.tq) * P.oc_ld + blk * 16, h, Bq.tq < T);
    }
    if (DROP) mst.load(P.dmask[0] + lw_off, bh, nt, 0, 0, true, tid);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int row = (t ? qb : qa) * 32 + r;
      u32x4 x[2];
      oc_tile(wf[0], hf[t][0], x);
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) *reinterpret_cast<u32x4*>(ks + row * G::RW + 16 * pr + 8 * h) = x[pr];
      oc_tile(wf[2], hf[t][2], x);
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) *reinterpret_cast<u32x4*>(vs + row * G::TW + 16 * pr + 8 * h) = x[pr];
      oc_tile(wf[1], hf[t][1], x);
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) (t ? Bq : A).qf[pr] = __builtin_bit_cast(bf16x8, x[pr]);
    }
    if (DROP) mst.store(msk, tid);
  }
  __syncthreads();
  A.m = -INFINITY; A.l = 0.f; Bq.m = -INFINITY; Bq.l = 0.f;
  zero16(A.o[0]);
  zero16(Bq.o[0]);
  {
    const uint32_t* mska = msk + (DROP ? w * MKT * 32 : 0);        // keep-bit tiles of qa, qb
    const uint32_t* mskb = msk + (DROP ? (7 - w) * MKT * 32 : 0);  // (key tile kt)
#define FWD_STEP(NQ, DA, DB, KT) \
  fwd_step<HS, NQ, DA, DB, DROP>(ks, vs, (KT) * 32, (KT) * 32, A, Bq, mska + (KT) * 32, mskb + (KT) * 32, c2, lane)
#define FWD_STEP_B(DB, KT) \
  fwd_step<HS, 1, DB, false, DROP>(ks, vs, (KT) * 32, (KT) * 32, Bq, A, mskb + (KT) * 32, mska, c2, lane)
    if (lb) {
      int kt = 0;
#pragma unroll 1
      for (; kt <= qa - 1; ++kt) FWD_STEP(2, false, false, kt);  // both tiles, off the diagonal
      FWD_STEP(2, true, false, qa);                              // tile a's diagonal
#pragma unroll 1
      for (kt = qa + 1; kt <= qb - 1; ++kt) FWD_STEP_B(false, kt);
      FWD_STEP_B(true, qb);
    } else if (la) {
#pragma unroll 1
      for (int kt = 0; kt <= qa - 1; ++kt) FWD_STEP(1, false, false, kt);
      FWD_STEP(1, true, false, qa);
    }
#undef FWD_STEP
#undef FWD_STEP_B
  }
  // normalise the outputs and keep the LSE (as attn_fwd_kernel's one-stream epilogue: 16-B row pieces after a
  // v_permlane32_swap of the two lane halves; the swaps run on every lane)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const bool live = u == 0 ? la : lb;
    FwdQ<HS>& q = u == 0 ? A : Bq;
    const float l = xhalf_sum(q.l);
    const float inv = (l > 0.f) ? (DROP ? P.drop_scale : 1.f) / l : 0.f;
    u32x4 ov[2];
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const int ga = 2 * pr, gb = 2 * pr + 1;
      const uint32_t x0 = pack2bf(q.o[0][4 * ga] * inv, q.o[0][4 * ga + 1] * inv);
      const uint32_t x1 = pack2bf(q.o[0][4 * ga + 2] * inv, q.o[0][4 * ga + 3] * inv);
      const uint32_t y0 = pack2bf(q.o[0][4 * gb] * inv, q.o[0][4 * gb + 1] * inv);
      const uint32_t y1 = pack2bf(q.o[0][4 * gb + 2] * inv, q.o[0][4 * gb + 3] * inv);
      const auto s0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
      ov[pr] = u32x4{s0[0], s1[0], s0[1], s1[1]};  // d = 16 pr + 8 h + 0..7
    }
    if (live && q.tq < T) {
      if (h == 0) P.lse[0][(int64_t)bh * T + q.tq] = q.m + __log2f(l);  // log2 domain
      bf16_t* dst = P.o + (rowbase + q.tq) * P.o_ld + head * HS;
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) *reinterpret_cast<u32x4*>(dst + 16 * pr + 8 * h) = ov[pr];
    }
  }
}


// launches the plan's on-chip-QKV forward (mmt_attn_plan checked the fields and sized the grid)
hipError_t mmt_attn_oc_launch_plan(const AttnBatch& b, const AttnLaunch& l, int T, int H, float scale, hipStream_t s) {
  const dim3 grid(l.gx, l.gy, l.gz), wg(l.wg);
  switch (attn_key(l)) {
#define X(D) \
  case attn_key(ATTN_OC32_FWD, 0, D): hipLaunchKernelGGL((attn_fwd_oc32_kernel<D>), grid, wg, 0, s, b, T, H, scale); break;
    ATTN_OC32_OPS(X)
#undef X
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
