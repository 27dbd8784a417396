// Causal self-attention and multi-stream selective cross-attention for gfx950.
//
// Reference semantics (model.py:60-73, 136-159): per head, aff = q k^T * hs^-0.5, causal mask,
// softmax, @ v. Cross-attention runs one independent causal softmax per KV modality ("stream")
// and SUMS the per-stream outputs (no joint softmax).
//
// Structure: a 256-thread workgroup (4 waves) owns 8 32-row tiles of one (batch, head) (wave w
// takes tiles w and 7-w: balanced causal work). The operand the tiles share (K/V in the forward
// and dQ pass, Q/dO/LSE/D in the dK/dV pass) is staged into LDS in chunks of up to 256 rows; at
// T <= chunk the whole sequence lands with one barrier (see "Chunked staging" below).
// All products are v_mfma_f32_32x32x16_bf16 with fp32 accumulation:
//   forward  S^T = K Q^T (keys on accumulator rows, queries on lanes) -> online softmax per lane;
//            O^T += V^T P^T with P^T straight from the accumulator registers as the B operand and
//            V^T by ds_read_b64_tr_b16 from the V tile.
//   dQ       S^T, dP^T recomputed per key tile; dQ^T += K^T dS^T (K^T by transposed LDS reads).
//   dK, dV   S = Q K^T, dP = dO V^T (queries on rows); dV += P^T dO, dK += dS^T Q with P and dS
//            taken from registers as the A operand and dO / Q by transposed LDS reads.
// Head sizes 8..64: padded to 16 on the reduction side and to 32 on the output side.
// Dropout (model.py:69, 151: applied to the normalised probabilities): a counter-hash mask,
// O = (P.Z) V with Z = mask / (1 - p), so dV = (P.Z)^T dO, dS = P.(Z.dP - D) with D = rowsum(dO.O)
// unchanged. The hash runs once, in attn_mask_kernel (launched on a side stream, overlapping the
// GEMMs before the attention), which stores one keep bit per element in the S^T accumulator order
// (AttnProblem::dmask). The three attention kernels stage the bits of their chunk in LDS next to
// K/V (Q/dO) and apply them with no hashing: the forward and dQ pass turn a pair of mask dwords
// into the lane mask of a v_cndmask (inverse ballot), the dK/dV pass (keys on lanes) extracts its
// bit per element. 1/(1-p) is folded into the output normalisation / dV write-out.
#include <stdlib.h>

#include <algorithm>

#include <type_traits>

#include "mmt_common.h"
#include "mmt_kernels.h"
#include "mmt_attn_plan.h"

#include "mmt_attn_dev.h"

// =============================================================================================
// forward: grid (ceil(nt/8) * B*H, 1, G). Wave w owns query tiles qa = 8*bx + w and qb = 8*bx + 7 - w
// and walks them TOGETHER: while both need a key tile the two online softmaxes run as one
// straight-line body (no branches: the diagonal and dropout variants are compile-time), so two
// independent MFMA -> softmax -> MFMA chains interleave in the wave; the resident K/V chunk of each
// (stream, chunk) is loaded once per block.
// =============================================================================================
template <int HS, bool DROP>
__global__ __launch_bounds__(256, MMT_FWD_MINB(HS)) void attn_fwd_kernel(AttnBatch batch, int T, int H, float scale) {
  using G = Geo<HS>;
  constexpr int ROWS = Chunk<HS>::ROWS;
  constexpr int MKT = ROWS / 32;     // key tiles per chunk
  constexpr int MDW = 8 * MKT * 32;  // keep-bit dwords per chunk
  const AttnProblem& P = batch.p[blockIdx.z];
  // grid.x = nb * B*H in XCD-aware logical order: the heads of one batch row (halves of the same
  // Q/K/V cache lines) run on one XCD together
  const int nb = ((T + 31) / 32 + 7) / 8;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int bh = tile / nb, b = bh / H, head = bh % H;
  const int bx = tile % nb;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int nt = (T + 31) / 32;
  const int qt0 = bx * 8;
  const int qmax = min(qt0 + 7, nt - 1);
  const int nch = (min((qmax + 1) * 32, T) + ROWS - 1) / ROWS;
  const int64_t rowbase = (int64_t)b * T;
  const float c2 = scale * kLog2e;
  __shared__ __attribute__((aligned(16))) bf16_t ks[ROWS * G::RW];
  __shared__ __attribute__((aligned(16))) bf16_t vs[ROWS * G::TW];
  using MS = MaskStager<HS>;
  __shared__ __attribute__((aligned(16))) uint32_t msk[DROP ? MDW : 4];  // keep-bit lane words
  // lane-word record of the keep bits (AttnProblem::dmask): after the key-major one
  const int BH = gridDim.x / nb;
  const int64_t lw_off = (int64_t)BH * (nt * (nt + 1) / 2) * 32;
  Stager<HS> st;
  MS mst;
  if (HS % 32 != 0) {  // pad columns are read only when HS is not a multiple of 32
    for (int q = tid; q < ROWS * G::RW; q += 256) if (q % G::RW >= HS) ks[q] = 0;
    for (int q = tid; q < ROWS * G::TW; q += 256) if (q % G::TW >= HS) vs[q] = 0;
  }
  st.load(P.k[0] + head * P.kv_hstride, P.kv_ld, P.v[0] + head * P.kv_hstride, P.kv_ld, rowbase, 0, T, tid);
  if (DROP) mst.load(P.dmask[0] + lw_off, bh, nt, qt0, 0, true, tid);
  st.store(ks, G::RW, vs, G::TW, tid);
  if (DROP) mst.store(msk, tid);

  const int qa = qt0 + w, qb = qt0 + 7 - w;  // qa < qb
  const bool la = qa < nt, lb = qb < nt;     // lb implies la
  FwdQ<HS> A, Bq;
  A.tq = qa * 32 + r;
  Bq.tq = qb * 32 + r;
#pragma unroll
  for (int s = 0; s < G::NKS; ++s) {
    const int d0 = 16 * s + 8 * h;
    A.qf[s] = ld8(P.q + (rowbase + A.tq) * P.q_ld + head * HS + d0, la && A.tq < T && d0 < HS);
    Bq.qf[s] = ld8(P.q + (rowbase + Bq.tq) * P.q_ld + head * HS + d0, lb && Bq.tq < T && d0 < HS);
  }
  __syncthreads();
  for (int j = 0; j < P.nstreams; ++j) {
    A.m = -INFINITY; A.l = 0.f; Bq.m = -INFINITY; Bq.l = 0.f;
#pragma unroll
    for (int dt = 0; dt < G::ND; ++dt) { zero16(A.o[dt]); zero16(Bq.o[dt]); }
    for (int c = 0; c < nch; ++c) {
      const uint32_t* mska = msk + (DROP ? w * MKT * 32 : 0);        // keep-bit tiles of qa, qb
      const uint32_t* mskb = msk + (DROP ? (7 - w) * MKT * 32 : 0);  // (chunk tile kt - kt_lo)
      const int kt_lo = c * MKT;
      const int kt_hi = min(kt_lo + MKT, nt) - 1;
#define FWD_STEP(NQ, DA, DB, KT) \
  fwd_step<HS, NQ, DA, DB, DROP>(ks, vs, ((KT) - kt_lo) * 32, (KT) * 32, A, Bq, mska + ((KT) - kt_lo) * 32, \
                                 mskb + ((KT) - kt_lo) * 32, c2, lane)
#define FWD_STEP_B(DB, KT) \
  fwd_step<HS, 1, DB, false, DROP>(ks, vs, ((KT) - kt_lo) * 32, (KT) * 32, Bq, A, mskb + ((KT) - kt_lo) * 32, \
                                   mska, c2, lane)
      if (lb) {
        int kt = kt_lo;
#pragma unroll 1
        for (; kt <= min(qa - 1, kt_hi); ++kt) FWD_STEP(2, false, false, kt);  // both tiles, off the diagonal
        if (qa >= kt_lo && qa <= kt_hi) FWD_STEP(2, true, false, qa);        // tile a's diagonal
#pragma unroll 1
        for (kt = max(kt_lo, qa + 1); kt <= min(qb - 1, kt_hi); ++kt) FWD_STEP_B(false, kt);
        if (qb >= kt_lo && qb <= kt_hi) FWD_STEP_B(true, qb);
      } else if (la) {
#pragma unroll 1
        for (int kt = kt_lo; kt <= min(qa - 1, kt_hi); ++kt) FWD_STEP(1, false, false, kt);
        if (qa >= kt_lo && qa <= kt_hi) FWD_STEP(1, true, false, qa);
      }
#undef FWD_STEP
#undef FWD_STEP_B
      // next (stream, chunk) resident for the whole block
      int nj = j, nc = c + 1;
      if (nc == nch) { nc = 0; ++nj; }
      if (nj < P.nstreams && (nj != j || nc != c)) {
        __syncthreads();
        st.load(P.k[nj] + head * P.kv_hstride, P.kv_ld, P.v[nj] + head * P.kv_hstride, P.kv_ld, rowbase, nc * ROWS,
                T, tid);
        if (DROP) mst.load(P.dmask[nj] + lw_off, bh, nt, qt0, nc * (ROWS / 32), true, tid);
        st.store(ks, G::RW, vs, G::TW, tid);
        if (DROP) mst.store(msk, tid);
        __syncthreads();
      }
    }
    // normalise this stream's outputs and keep its LSE. One stream: the output itself; several:
    // each stream's own output (the backward reads it), summed below
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bool live = u == 0 ? la : lb;
      FwdQ<HS>& q = u == 0 ? A : Bq;
      const float l = xhalf_sum(q.l);
      const float inv = (l > 0.f) ? (DROP ? P.drop_scale : 1.f) / l : 0.f;
      // row-per-lane O^T halves (lane r: d 8g..8g+3, lane r + 32: 8g+4..8g+7) exchanged across the
      // wave halves by v_permlane32_swap so every lane holds 8 consecutive d of its row: 16-B stores,
      // half the store instructions of the 8-B form (the epilogue store tail is issue-bound). The
      // swaps run on every lane (both halves of a row are live or dead together).
      u32x4 ov[G::ND][2];
#pragma unroll
      for (int dt = 0; dt < G::ND; ++dt)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          const int ga = 2 * pr, gb = 2 * pr + 1;
          const uint32_t x0 = pack2bf(q.o[dt][4 * ga] * inv, q.o[dt][4 * ga + 1] * inv);
          const uint32_t x1 = pack2bf(q.o[dt][4 * ga + 2] * inv, q.o[dt][4 * ga + 3] * inv);
          const uint32_t y0 = pack2bf(q.o[dt][4 * gb] * inv, q.o[dt][4 * gb + 1] * inv);
          const uint32_t y1 = pack2bf(q.o[dt][4 * gb + 2] * inv, q.o[dt][4 * gb + 3] * inv);
          const auto s0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
          ov[dt][pr] = u32x4{s0[0], s1[0], s0[1], s1[1]};  // d = dt*32 + 16 pr + 8 h + 0..7
        }
      if (live && q.tq < T) {
        if (h == 0) P.lse[j][(int64_t)bh * T + q.tq] = q.m + __log2f(l);  // log2 domain
        bf16_t* dst = (P.nstreams > 1 ? P.oj[j] : P.o) + (rowbase + q.tq) * P.o_ld + head * HS;
#pragma unroll
        for (int dt = 0; dt < G::ND; ++dt)
#pragma unroll
          for (int pr = 0; pr < 2; ++pr) {
            const int d0 = dt * 32 + 16 * pr + 8 * h;
            if (d0 < HS) *reinterpret_cast<u32x4*>(dst + d0) = ov[dt][pr];
          }
      }
    }
  }
  // several streams: the output is the sum of the per-stream outputs this lane just wrote (kept
  // out of registers: a running fp32 total would pin another O-sized accumulator set)
  if (P.nstreams > 1) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bool live = u == 0 ? la : lb;
      const int tq = u == 0 ? A.tq : Bq.tq;
      if (!(live && tq < T)) continue;
      const int64_t off = (rowbase + tq) * P.o_ld + head * HS;
#pragma unroll
      for (int dt = 0; dt < G::ND; ++dt)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          const int d0 = dt * 32 + 16 * pr + 8 * h;  // the 16-B pieces this lane wrote
          if (d0 >= HS) continue;
          float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          for (int jj = 0; jj < P.nstreams; ++jj) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(P.oj[jj] + off + d0);
#pragma unroll
            for (int e = 0; e < 4; ++e) { t[2 * e] += bf2f(v[e] & 0xffff); t[2 * e + 1] += bf2f(v[e] >> 16); }
          }
          *reinterpret_cast<u32x4*>(P.o + off + d0) =
              u32x4{pack2bf(t[0], t[1]), pack2bf(t[2], t[3]), pack2bf(t[4], t[5]), pack2bf(t[6], t[7])};
        }
    }
  }
}

// per query tile state of the dQ walk: Q / dO fragments, the row's log2-domain LSE and D, dQ^T
template <int HS>
struct DqQ {
  bf16x8 qf[Geo<HS>::NKS], dof[Geo<HS>::NKS];
  f32x16 dq[Geo<HS>::ND];
  float lse2, dsum;
  int tq;
};

// dS^T of one tile for one query tile (in place in sacc), packed to the two bf16 operand fragments
template <int HS, bool diag, bool DROP>
__device__ __forceinline__ void dq_ds(f32x16& sacc, const f32x16& dpacc, const DqQ<HS>& q, int k0, float c2,
                                      float dsc, uint32_t mw, int h, bf16x8 (&df)[2]) {
  const float nl = -q.lse2, nd = -q.dsum;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    float pv = ex2(__builtin_fmaf(sacc[e], c2, nl));
    if (diag) {
      const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (key > q.tq) pv = 0.f;
    }
    float dp = dpacc[e];
    if (DROP) dp = keep_f(dp, elem_keep(mw, e));
    sacc[e] = pv * __builtin_fmaf(dp, dsc, nd);  // dS^T = P (Z.dP - D) (dropped: -P D)
  }
  df[0] = acc_frag(sacc, 0);
  df[1] = acc_frag(sacc, 1);
}

// dQ step over one 32-key tile for one or two query tiles: S^T, dP^T recomputed, dQ^T += K^T dS^T.
// The K / V row fragments and the transposed K fragments are read once for both tiles and issued
// up front (the transposed ones land behind the dS arithmetic)
template <int HS, int NQ, bool DA, bool DB, bool DROP>
__device__ __forceinline__ void dq_step(const bf16_t* ks, const bf16_t* vs, const bf16_t* kts, int kts_ld, int kl,
                                        int k0, DqQ<HS>& a, DqQ<HS>& b, const uint32_t* mta, const uint32_t* mtb,
                                        float c2, const AttnProblem& P, int lane) {
  using G = Geo<HS>;
  const int r = lane & 31, h = lane >> 5;
  const uint32_t wa = DROP ? reinterpret_cast<const uint16_t*>(mta)[lane] : 0u;  // keep bits (LDS)
  const uint32_t wb = (DROP && NQ == 2) ? reinterpret_cast<const uint16_t*>(mtb)[lane] : 0u;
  f32x16 sa, pa, sb, pb;
  zero16(sa);
  zero16(pa);
  if (NQ == 2) { zero16(sb); zero16(pb); }
  constexpr bool SL = SliceImg<HS>::on;
  if (NQ == 2) {
    bf16x8 kf[G::NKS], vf[G::NKS];
#pragma unroll
    for (int s = 0; s < G::NKS; ++s) {
      kf[s] = SL ? sl_row(ks, kl, r, s, h) : *reinterpret_cast<const bf16x8*>(ks + (kl + r) * G::RW + 16 * s + 8 * h);
      vf[s] = SL ? sl_row(vs, kl, r, s, h) : *reinterpret_cast<const bf16x8*>(vs + (kl + r) * G::RW + 16 * s + 8 * h);
    }
#pragma unroll
    for (int s = 0; s < G::NKS; ++s) {
      sa = mfma32(kf[s], a.qf[s], sa);
      pa = mfma32(vf[s], a.dof[s], pa);
      sb = mfma32(kf[s], b.qf[s], sb);
      pb = mfma32(vf[s], b.dof[s], pb);
    }
  } else {  // register-lean order (hs >= 48)
#pragma unroll
    for (int s = 0; s < G::NKS; ++s) {
      const bf16x8 kf = SL ? sl_row(ks, kl, r, s, h) : *reinterpret_cast<const bf16x8*>(ks + (kl + r) * G::RW + 16 * s + 8 * h);
      const bf16x8 vf = SL ? sl_row(vs, kl, r, s, h) : *reinterpret_cast<const bf16x8*>(vs + (kl + r) * G::RW + 16 * s + 8 * h);
      sa = mfma32(kf, a.qf[s], sa);
      pa = mfma32(vf, a.dof[s], pa);
    }
  }
  const float dsc = DROP ? P.drop_scale : 1.f;
  bf16x8 dfa[2], dfb[2];
  if (NQ == 2) {
    bf16x8 kt[2][G::ND];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int dt = 0; dt < G::ND; ++dt) kt[s][dt] = SL ? sl_tr(kts, kl, s, lane) : tr_frag(kts + kl * kts_ld, kts_ld, dt, s, lane);
    dq_ds<HS, DA, DROP>(sa, pa, a, k0, c2, dsc, wa, h, dfa);
    dq_ds<HS, DB, DROP>(sb, pb, b, k0, c2, dsc, wb, h, dfb);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int dt = 0; dt < G::ND; ++dt) {
        a.dq[dt] = mfma32(kt[s][dt], dfa[s], a.dq[dt]);
        b.dq[dt] = mfma32(kt[s][dt], dfb[s], b.dq[dt]);
      }
  } else {
    dq_ds<HS, DA, DROP>(sa, pa, a, k0, c2, dsc, wa, h, dfa);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int dt = 0; dt < G::ND; ++dt)
        a.dq[dt] = mfma32(SL ? sl_tr(kts, kl, s, lane) : tr_frag(kts + kl * kts_ld, kts_ld, dt, s, lane), dfa[s], a.dq[dt]);
  }
}

// =============================================================================================
// backward dQ (also writes D_j = rowsum(dO * O_j) for the dK/dV pass); grid as forward, and like the
// forward each wave walks its two query tiles together
// =============================================================================================
template <int HS, bool DROP>
__global__ __launch_bounds__(256, MMT_DQ_MINB(HS)) void attn_bwd_dq_kernel(AttnBatch batch, int T, int H,
                                                                                       float scale) {
  using G = Geo<HS>;
  // chunk rows: hs >= 48 stages 256-row chunks (two 128-row register rounds; 80 KB of LDS, still two
  // blocks per CU, which is what the registers allow): half the reloads and barriers of 128-row
  // chunks, and at T = 512 each chunk holds either a whole causal triangle or a full rectangle, so
  // the four waves' work per chunk is balanced
  constexpr int SR = Chunk<HS>::ROWS;
  constexpr int ROWS = HS >= 48 ? 256 : SR;
  constexpr int NR = ROWS / SR;
  const AttnProblem& P = batch.p[blockIdx.z];
  const int nb = ((T + 31) / 32 + 7) / 8;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int bh = tile / nb, b = bh / H, head = bh % H;
  const int bx = tile % nb;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int nt = (T + 31) / 32;
  const int qt0 = bx * 8;
  const int qmax = min(qt0 + 7, nt - 1);
  const int nch = (min((qmax + 1) * 32, T) + ROWS - 1) / ROWS;
  const int64_t rowbase = (int64_t)b * T;
  const float c2 = scale * kLog2e;
  __shared__ __attribute__((aligned(16))) bf16_t ks[ROWS * G::RW];  // K chunk: row (+ tr at hs > 32) reads
  __shared__ __attribute__((aligned(16))) bf16_t vs[ROWS * G::RW];  // V chunk: row reads
  const bf16_t* kts = ks;
  constexpr int KTS_LD = G::RW;
  using MS = MaskStager<HS, ROWS / 32>;
  __shared__ __attribute__((aligned(16))) uint32_t msk[DROP ? MS::DWORDS : 4];  // keep-bit lane words
  if (HS % 32 != 0) {  // pad columns are read only when HS is not a multiple of 32
    for (int q = tid; q < ROWS * G::RW; q += 256)
      if (q % G::RW >= HS) { ks[q] = 0; vs[q] = 0; }
  }
  Stager<HS> st;
  MS mst;
  // lane-word record of the keep bits (AttnProblem::dmask): after the key-major one
  const int64_t lw_off = (int64_t)(gridDim.x / nb) * (nt * (nt + 1) / 2) * 32;
  auto stage = [&](int jj, int cc) {  // K / V rows [cc*ROWS, +ROWS) of stream jj and their keep bits
    if (DROP) mst.load(P.dmask[jj] + lw_off, bh, nt, qt0, cc * (ROWS / 32), true, tid);
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) {
      st.load(P.k[jj] + head * P.kv_hstride, P.kv_ld, P.v[jj] + head * P.kv_hstride, P.kv_ld, rowbase,
              cc * ROWS + rr * SR, T, tid);
      if constexpr (SliceImg<HS>::on) st.store_slices(ks + rr * SR * G::RW, vs + rr * SR * G::RW, tid);
      else st.store(ks + rr * SR * G::RW, G::RW, vs + rr * SR * G::RW, G::RW, tid);
    }
    if (DROP) mst.store(msk, tid);
  };
  stage(0, 0);
  __syncthreads();

  const int qa = qt0 + w, qb = qt0 + 7 - w;  // qa < qb; lb implies la
  const bool la = qa < nt, lb = qb < nt;
  const uint32_t* mska = msk + (DROP ? w * MS::KT * 32 : 0);        // keep-bit tiles of qa, qb
  const uint32_t* mskb = msk + (DROP ? (7 - w) * MS::KT * 32 : 0);  // (chunk tile kt - kt_lo)
  DqQ<HS> A, Bq;
  A.tq = qa * 32 + r;
  Bq.tq = qb * 32 + r;
  const bool oka = la && A.tq < T, okb = lb && Bq.tq < T;
#pragma unroll
  for (int s = 0; s < G::NKS; ++s) {
    const int d0 = 16 * s + 8 * h;
    A.qf[s] = ld8(P.q + (rowbase + A.tq) * P.q_ld + head * HS + d0, oka && d0 < HS);
    A.dof[s] = ld8(P.dout + (rowbase + A.tq) * P.dout_ld + head * HS + d0, oka && d0 < HS);
    Bq.qf[s] = ld8(P.q + (rowbase + Bq.tq) * P.q_ld + head * HS + d0, okb && d0 < HS);
    Bq.dof[s] = ld8(P.dout + (rowbase + Bq.tq) * P.dout_ld + head * HS + d0, okb && d0 < HS);
  }
#pragma unroll
  for (int dt = 0; dt < G::ND; ++dt) { zero16(A.dq[dt]); zero16(Bq.dq[dt]); }
  for (int j = 0; j < P.nstreams; ++j) {
    const bf16_t* oj = (P.nstreams > 1) ? P.oj[j] : P.o;
    float dsa = 0.f, dsb = 0.f;
#pragma unroll
    for (int s = 0; s < G::NKS; ++s) {
      const int d0 = 16 * s + 8 * h;
      const bf16x8 ova = ld8(oj + (rowbase + A.tq) * P.o_ld + head * HS + d0, oka && d0 < HS);
      const bf16x8 ovb = ld8(oj + (rowbase + Bq.tq) * P.o_ld + head * HS + d0, okb && d0 < HS);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        dsa += (float)ova[e] * (float)A.dof[s][e];
        dsb += (float)ovb[e] * (float)Bq.dof[s][e];
      }
    }
    dsa = xhalf_sum(dsa);
    dsb = xhalf_sum(dsb);
    if (h == 0) {  // D_j / drop_scale for the dK/dV pass (dkdv_tile: dS = sc (Z P dP - P D / sc))
      const float inv = DROP ? 1.0f / P.drop_scale : 1.0f;
      if (oka) P.dvec[j][(int64_t)bh * T + A.tq] = dsa * inv;
      if (okb) P.dvec[j][(int64_t)bh * T + Bq.tq] = dsb * inv;
    }
    A.dsum = dsa;
    Bq.dsum = dsb;
    A.lse2 = oka ? P.lse[j][(int64_t)bh * T + A.tq] : 0.f;
    Bq.lse2 = okb ? P.lse[j][(int64_t)bh * T + Bq.tq] : 0.f;
    for (int c = 0; c < nch; ++c) {
      const int kt_lo = c * (ROWS / 32);
      const int kt_hi = min(kt_lo + ROWS / 32, nt) - 1;
#define DQ_STEP(NQ, DA, DB, KT) \
  dq_step<HS, NQ, DA, DB, DROP>(ks, vs, kts, KTS_LD, ((KT) - kt_lo) * 32, (KT) * 32, A, Bq, mska + ((KT) - kt_lo) * 32, \
                                mskb + ((KT) - kt_lo) * 32, c2, P, lane)
#define DQ_STEP_B(DB, KT) \
  dq_step<HS, 1, DB, false, DROP>(ks, vs, kts, KTS_LD, ((KT) - kt_lo) * 32, (KT) * 32, Bq, A, mskb + ((KT) - kt_lo) * 32, mska, \
                                  c2, P, lane)
      if (lb) {
        int kt = kt_lo;
        // hs >= 48: the two tiles' S / dP accumulators do not fit beside their Q / dO / dQ state
        // (two waves per SIMD), so the tiles take turns (each re-reads the K / V fragments)
        constexpr int NQ2 = HS >= 48 ? 1 : 2;
#pragma unroll 1
        for (; kt <= min(qa - 1, kt_hi); ++kt) {
          DQ_STEP(NQ2, false, false, kt);
          if (NQ2 == 1) DQ_STEP_B(false, kt);
        }
        if (qa >= kt_lo && qa <= kt_hi) {
          DQ_STEP(NQ2, true, false, qa);
          if (NQ2 == 1) DQ_STEP_B(false, qa);
        }
#pragma unroll 1
        for (kt = max(kt_lo, qa + 1); kt <= min(qb - 1, kt_hi); ++kt) DQ_STEP_B(false, kt);
        if (qb >= kt_lo && qb <= kt_hi) DQ_STEP_B(true, qb);
      } else if (la) {
#pragma unroll 1
        for (int kt = kt_lo; kt <= min(qa - 1, kt_hi); ++kt) DQ_STEP(1, false, false, kt);
        if (qa >= kt_lo && qa <= kt_hi) DQ_STEP(1, true, false, qa);
      }
#undef DQ_STEP
#undef DQ_STEP_B
      int nj = j, nc = c + 1;
      if (nc == nch) { nc = 0; ++nj; }
      if (nj < P.nstreams && (nj != j || nc != c)) {
        __syncthreads();
        stage(nj, nc);
        __syncthreads();
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const bool ok = u == 0 ? oka : okb;
    const DqQ<HS>& q = u == 0 ? A : Bq;
    // 16-B stores of 8 consecutive d per lane after a v_permlane32_swap exchange of the row halves
    // (as the forward's O); the swaps run on every lane
    u32x4 dv[G::ND][2];
#pragma unroll
    for (int dt = 0; dt < G::ND; ++dt)
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        const int ga = 2 * pr, gb = 2 * pr + 1;
        const uint32_t x0 = pack2bf(q.dq[dt][4 * ga] * scale, q.dq[dt][4 * ga + 1] * scale);
        const uint32_t x1 = pack2bf(q.dq[dt][4 * ga + 2] * scale, q.dq[dt][4 * ga + 3] * scale);
        const uint32_t y0 = pack2bf(q.dq[dt][4 * gb] * scale, q.dq[dt][4 * gb + 1] * scale);
        const uint32_t y1 = pack2bf(q.dq[dt][4 * gb + 2] * scale, q.dq[dt][4 * gb + 3] * scale);
        const auto s0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
        dv[dt][pr] = u32x4{s0[0], s1[0], s0[1], s1[1]};
      }
    if (ok) {
#pragma unroll
      for (int dt = 0; dt < G::ND; ++dt)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          const int d0 = dt * 32 + 16 * pr + 8 * h;
          if (d0 < HS) *reinterpret_cast<u32x4*>(P.dq + (rowbase + q.tq) * P.dq_ld + head * HS + d0) = dv[dt][pr];
        }
    }
  }
}

// dK, dV: one 32x32 (queries x keys) tile; S, dP recomputed, dV += P^T dO, dK += dS^T Q
template <int HS, bool MASKED, bool DROP>
__device__ __forceinline__ void dkdv_tile(const bf16_t* qs, const bf16_t* dos, const float* lsl, const float* dsl,
                                          int ql, int q0, int tk, int T,
                                          const bf16x8 (&kf)[Geo<HS>::NKS], const bf16x8 (&vf)[Geo<HS>::NKS],
                                          f32x16 (&dk)[Geo<HS>::ND], f32x16 (&dv)[Geo<HS>::ND], float c2,
                                          const AttnProblem& P, const uint32_t* mt, int lane) {
  using G = Geo<HS>;
  const int r = lane & 31, h = lane >> 5;
  // key r's keep bits over the tile's queries, this lane's half (queries 8g + 4h + e4) at bits 8g + e4
  const uint32_t mw = DROP ? mt[key_dword(r)] >> (4 * h) : 0u;
  f32x16 sacc, dpacc;
  zero16(sacc);
  zero16(dpacc);
  // every LDS read of the tile is issued up front, in the order it is consumed (row fragments for
  // S and dP, then the transposed Q / dO fragments for dK / dV behind the softmax VALU): the
  // compiler then waits on counted lgkmcnt instead of a read -> wait -> MFMA chain per fragment
  bf16x8 qr[G::NKS], dr[G::NKS];
  constexpr bool SL = SliceImg<HS>::on;
#pragma unroll
  for (int s = 0; s < G::NKS; ++s) {
    qr[s] = SL ? sl_row(qs, ql, r, s, h) : *reinterpret_cast<const bf16x8*>(qs + (ql + r) * G::RW + 16 * s + 8 * h);
    dr[s] = SL ? sl_row(dos, ql, r, s, h) : *reinterpret_cast<const bf16x8*>(dos + (ql + r) * G::RW + 16 * s + 8 * h);
  }
#pragma unroll
  for (int s = 0; s < G::NKS; ++s) {
    sacc = mfma32(qr[s], kf[s], sacc);    // S[q][key]
    dpacc = mfma32(dr[s], vf[s], dpacc);  // dP[q][key]
  }
  bf16x8 dot[2][G::ND], qtr[2][G::ND];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int dt = 0; dt < G::ND; ++dt) {
      dot[s][dt] = SL ? sl_tr(dos, ql, s, lane) : tr_frag(dos + ql * G::RW, G::RW, dt, s, lane);
      qtr[s][dt] = SL ? sl_tr(qs, ql, s, lane) : tr_frag(qs + ql * G::RW, G::RW, dt, s, lane);
    }
  f32x4 l4[4], d4[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    l4[g] = *reinterpret_cast<const f32x4*>(lsl + ql + 8 * g + 4 * h);
    d4[g] = *reinterpret_cast<const f32x4*>(dsl + ql + 8 * g + 4 * h);
  }
  uint32_t pp[8], dd[8];  // packed bf16 pairs of Z.P (dV operand) and dS (dK operand)
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int e4 = 0; e4 < 4; e4 += 2) {
      float pm[2], ds[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int e = 4 * g + e4 + u;
        float pv = ex2(__builtin_fmaf(sacc[e], c2, l4[g][e4 + u]));
        if (MASKED) {
          const int tq = q0 + 8 * g + 4 * h + e4 + u;
          if (!(tk <= tq && tq < T)) pv = 0.f;
        }
        const float dp = dpacc[e];
        if (DROP) {
          // Z.P without the 1/(1-p) (applied to dV at the end); dS = P (Z dP sc - D) = sc (Z P dP - P D'),
          // D' = D / sc (the dQ pass stores it so), the factor sc applied to dK at the end: one VALU
          // per element fewer than masking dP separately
          int kb = __builtin_amdgcn_sbfe((int)mw, 8 * g + e4 + u, 1);  // all ones iff kept
          // (opaque to the compiler: seen as a one-bit test it lowered bfe + and into and + cmp + cndmask)
          asm volatile("" : "+v"(kb));
          pm[u] = keep_f(pv, kb);
          ds[u] = __builtin_fmaf(pm[u], dp, pv * d4[g][e4 + u]);  // dS[q][key] / sc
        } else {
          pm[u] = pv;
          ds[u] = pv * (dp + d4[g][e4 + u]);  // dS[q][key]
        }
      }
      pp[2 * g + e4 / 2] = pack2bf(pm[0], pm[1]);
      dd[2 * g + e4 / 2] = pack2bf(ds[0], ds[1]);
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x8 pf = __builtin_bit_cast(bf16x8, u32x4{pp[4 * s], pp[4 * s + 1], pp[4 * s + 2], pp[4 * s + 3]});
    const bf16x8 df = __builtin_bit_cast(bf16x8, u32x4{dd[4 * s], dd[4 * s + 1], dd[4 * s + 2], dd[4 * s + 3]});
#pragma unroll
    for (int dt = 0; dt < G::ND; ++dt) {
      dv[dt] = mfma32(pf, dot[s][dt], dv[dt]);
      dk[dt] = mfma32(df, qtr[s][dt], dk[dt]);
    }
  }
}

// Block-uniform walk over (tile u, stream j, chunk c): the chunk (j, c) resident in LDS is reused
// while consecutive steps share it (T <= ROWS with one stream: a single load for the whole block).
struct ChunkWalk {
  int ns, nch;
  __device__ __forceinline__ bool next(int u, int j, int c, int& nj, int& nc) const {
    nj = j; nc = c + 1;
    int nu = u;
    if (nc == nch) { nc = 0; ++nj; if (nj == ns) { nj = 0; ++nu; } }
    return nu < 2 && (nj != j || nc != c);
  }
};

// =============================================================================================
// backward dK, dV: grid (ceil(nt/8), B*H*nstreams, G); wave w owns key tiles 8*bx + w, 8*bx + 7 - w
// =============================================================================================
template <int HS, bool DROP>
__global__ __launch_bounds__(256, MMT_DKDV1_MINB(HS)) void attn_bwd_dkdv1_kernel(AttnBatch batch, int T, int H, float scale) {
  using G = Geo<HS>;
  constexpr int ROWS = Chunk<HS>::ROWS;
  const AttnProblem& P = batch.p[blockIdx.z];
  const int nb = ((T + 31) / 32 + 7) / 8;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int yy = tile / nb, bx = tile % nb;
  const int nbh = gridDim.x / nb / P.nstreams;
  if (yy >= nbh * P.nstreams) return;
  const int j = yy / nbh;
  const int bh = yy % nbh;
  const int b = bh / H, head = bh % H;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int nt = (T + 31) / 32;
  const int kt0 = bx * 8;
  const int q_lo = kt0 * 32;
  const ChunkWalk walk{1, (T - q_lo + ROWS - 1) / ROWS};
  const bool ragged = (T & 31) != 0;
  const int qlast = ragged ? nt - 1 : nt;  // the ragged last query tile (masked); nt: none
  const int64_t rowbase = (int64_t)b * T;
  const float c2 = scale * kLog2e;
  __shared__ __attribute__((aligned(16))) bf16_t qs[ROWS * G::RW];   // Q chunk: row + tr reads
  __shared__ __attribute__((aligned(16))) bf16_t dos[ROWS * G::RW];  // dO chunk: row + tr reads
  __shared__ __attribute__((aligned(16))) float lsd[2][ROWS];        // -log2-domain LSE, -D of the chunk rows
  using MS = MaskStager<HS>;
  __shared__ __attribute__((aligned(16))) uint32_t msk[DROP ? MS::DWORDS : 4];  // [key tile][chunk q tile]
  // epilogue transpose slots, one 32-column slice at a time: per wave [dK, dV][32 keys][EPW]
  constexpr int EPW = 40;
  __shared__ __attribute__((aligned(16))) bf16_t ept[4 * 2 * 32 * EPW];
  if (HS % 32 != 0)  // pad columns are read only when HS is not a multiple of 32
    for (int q = tid; q < ROWS * G::RW; q += 256)
      if (q % G::RW >= HS) { qs[q] = 0; dos[q] = 0; }

  const bf16_t* kp = P.k[j] + head * P.kv_hstride;
  const bf16_t* vp = P.v[j] + head * P.kv_hstride;
  const float* lsep = P.lse[j] + (int64_t)bh * T;
  const float* dvp = P.dvec[j] + (int64_t)bh * T;
  const bf16_t* qp = P.q + head * HS;
  const bf16_t* dop = P.dout + head * HS;
  constexpr int NSL = 2 * ROWS / 256;
  Stager<HS> st;
  MS mst;
  float sl[NSL];
  auto load = [&](int r0) {
    st.load(qp, P.q_ld, dop, P.dout_ld, rowbase, r0, T, tid);
    if (DROP) mst.load(P.dmask[j], bh, nt, kt0, r0 / 32, false, tid);
#pragma unroll
    for (int u = 0; u < NSL; ++u) {
      const int c = tid + 256 * u;
      const int t = r0 + (c % ROWS);
      sl[u] = t < T ? ((c < ROWS) ? -lsep[t] : -dvp[t]) : 0.f;  // negated: fma addends
    }
  };
  auto store = [&]() {
    if constexpr (SliceImg<HS>::on) st.store_slices(qs, dos, tid);
    else st.store(qs, G::RW, dos, G::RW, tid);
    if (DROP) mst.store(msk, tid);
#pragma unroll
    for (int u = 0; u < NSL; ++u) {
      const int c = tid + 256 * u;
      lsd[c / ROWS][c % ROWS] = sl[u];
    }
  };
  load(q_lo);
  store();
  __syncthreads();

#pragma unroll 1
  for (int u = 0; u < 2; ++u) {
    const int kt = u == 0 ? kt0 + w : kt0 + 7 - w;
    const bool live = kt < nt;
    const int tk = kt * 32 + r;
    bf16x8 kf[G::NKS], vf[G::NKS];
    f32x16 dk[G::ND], dv[G::ND];
#pragma unroll
    for (int s = 0; s < G::NKS; ++s) {
      const int d0 = 16 * s + 8 * h;
      const bool ok = live && tk < T && d0 < HS;
      kf[s] = ld8(kp + (rowbase + tk) * P.kv_ld + d0, ok);
      vf[s] = ld8(vp + (rowbase + tk) * P.kv_ld + d0, ok);
    }
#pragma unroll
    for (int dt = 0; dt < G::ND; ++dt) { zero16(dk[dt]); zero16(dv[dt]); }
    for (int c = 0; c < walk.nch; ++c) {
      int nj, nc;
      const bool reload = walk.next(u, 0, c, nj, nc);
      const int r0 = q_lo + c * ROWS;
      if (live) {
        const int qt_lo = r0 / 32, qt_hi = min(qt_lo + ROWS / 32, nt) - 1;
        const uint32_t* mk = msk + (kt - kt0) * MS::KT * 32;
        auto tile = [&](auto mc, int qt) {
          dkdv_tile<HS, decltype(mc)::value, DROP>(qs, dos, lsd[0], lsd[1], qt * 32 - r0, qt * 32, tk, T, kf, vf, dk, dv,
                                                   c2, P, mk + (qt - qt_lo) * 32, lane);
        };
        int qt = max(kt, qt_lo);  // diagonal and ragged last tile masked, peeled (see the paired kernel)
        if (qt == kt && qt <= qt_hi) tile(std::true_type{}, qt++);
        const int qe = min(qt_hi, qlast - 1);
#pragma unroll 1
        for (; qt <= qe; ++qt) tile(std::false_type{}, qt);
        if (qt <= qt_hi) tile(std::true_type{}, qt);
      }
      if (reload) {
        __syncthreads();
        load(q_lo + nc * ROWS);
        store();
        __syncthreads();
      }
    }
    // dK/dV tiles: accumulator rows = key ((e&3)+8(e>>2)+4h), cols = d (lane). Each 32-column slice
    // is transposed through this wave's LDS slot (ds_write_b16 at immediate offsets) and leaves as
    // row-major 16-B pieces: 2 dwordx4 per lane per matrix and slice instead of 16 two-byte stores
    // with a 64-bit address computation each
    if (live) {
      bf16_t* et = ept + w * (2 * 32 * EPW);
      const int k0 = kt * 32;
      const float dks = DROP ? scale * P.drop_scale : scale;  // dS was accumulated divided by drop_scale
#pragma unroll
      for (int dt = 0; dt < G::ND; ++dt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int kr = (e & 3) + 8 * (e >> 2) + 4 * h;
          et[kr * EPW + r] = f2bf(dk[dt][e] * dks);
          et[32 * EPW + kr * EPW + r] = f2bf(DROP ? dv[dt][e] * P.drop_scale : dv[dt][e]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = i * 16 + (lane >> 2), d0 = dt * 32 + (lane & 3) * 8;
          const u32x4 vk = *reinterpret_cast<const u32x4*>(et + row * EPW + (lane & 3) * 8);
          const u32x4 vv = *reinterpret_cast<const u32x4*>(et + 32 * EPW + row * EPW + (lane & 3) * 8);
          if (k0 + row < T && d0 < HS) {
            const int64_t off = (rowbase + k0 + row) * P.dkv_ld + d0;
            *reinterpret_cast<u32x4*>(P.dk[j] + head * P.dkv_hstride + off) = vk;
            *reinterpret_cast<u32x4*>(P.dv[j] + head * P.dkv_hstride + off) = vv;
          }
        }
      }
    }
  }
}

// =============================================================================================
// One-pass backward at hs 32 for T <= 256 and one KV stream (C1's self-attention; round 6).
// grid (B*H, 1, problems): one workgroup (4 waves; two workgroups per CU) per (batch, head) owns all
// nt <= 8 key tiles, so S and dP -- and their softmax / dropout VALU -- are computed ONCE per tile
// (the two-pass kernels above recompute both in the dQ pass: 14 products per tile instead of 10)
// and dQ needs no sum across workgroups:
//  * Q and dO of the whole sequence land in LDS by LDS-DMA as slice images (SliceImg: conflict-free
//    row AND transposed reads); D = rowsum(dO O) and the negated log2-domain LSE of every query go
//    into LDS tables (thread t: query t);
//  * wave w owns key tiles w and 7 - w (9 tile pairs of the causal walk each at nt = 8): their K / V
//    rows (keys on lanes: the B operands of S and dP) and K^T (the A operand of dQ, transposed once
//    through the wave's LDS slot) stay in registers, and so do their dK / dV accumulators;
//  * all waves walk the query tiles in step, one barrier per tile: for each owned key tile kt <= qt,
//    S = Q K^T, dP = dO V^T, P = exp2(c2 S - LSE2), dS = P (Z dP - D); dV += (Z P)^T dO and
//    dK += dS^T Q take P and dS straight from the accumulators as A operands (keys on lanes); dS
//    crosses the wave's LDS slot once and dQ_w^T += K^T dS^T runs on MFMA;
//  * each wave's fp32 dQ partial of the step goes to an LDS tile (double-buffered by step parity, so
//    one barrier per step suffices); after the barrier wave w sums rows 8w .. 8w+7 over the waves
//    that had tiles, scales, converts and stores them.
// LDS 78 KiB (two workgroups per CU): Q / dO images 2 x 18 KiB, tables 2 KiB, slots 4 x 2 KiB, dQ
// partials 2 x 4 x 4 KiB. dS is accumulated divided by the dropout scale sc (as the dK/dV pass:
// dS / sc = Z P dP - P D'), so dK and dQ take the factor sc at the end.
// The alternatives that were measured and lost (a walk without per-step barriers, a two-tile body,
// separate masked / unmasked bodies, a reversed walk in every second workgroup) are recorded with
// their numbers in DESIGN.md section 3, round 6.
// =============================================================================================
namespace {
typedef int32_t ai32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ ai32x4 a_rsrc(const void* base, int64_t bytes) {
  const uint64_t a = (uint64_t)base;
  ai32x4 rs;
  rs[0] = __builtin_amdgcn_readfirstlane((int32_t)(uint32_t)a);
  rs[1] = __builtin_amdgcn_readfirstlane((int32_t)((a >> 32) & 0xffffu));
  rs[2] = __builtin_amdgcn_readfirstlane((int32_t)min(bytes, (int64_t)0x7ffffff0));
  rs[3] = 0x00020000;
  return rs;
}
__device__ __forceinline__ uint32_t a_lds_u32(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)(p);
}
// 16 B per lane: LDS[lds + 16 lane] = buffer[voff] (zeros when voff is out of range)
__device__ __forceinline__ void a_dma16(const ai32x4& rsrc, uint32_t lds, int voff) {
  asm volatile("s_mov_b32 m0, %0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(lds), "v"(voff), "s"(rsrc)
               : "memory", "m0");
}
// 8 B per lane: buffer[voff] = v (dropped when voff is out of range): one store instruction whatever
// the lanes' rows, so counted vmcnt waits can include it
__device__ __forceinline__ void a_bst8(const ai32x4& rsrc, int voff, u32x2 v) {
  asm volatile("buffer_store_dwordx2 %0, %1, %2, 0 offen" : : "v"(v), "v"(voff), "s"(rsrc) : "memory");
}
__device__ __forceinline__ void a_bst16(const ai32x4& rsrc, int voff, f32x4 v) {
  asm volatile("buffer_store_dwordx4 %0, %1, %2, 0 offen" : : "v"(v), "v"(voff), "s"(rsrc) : "memory");
}
// counted wait on this wave's outstanding vector-memory operations (immediate operand, n <= 8)
__device__ __forceinline__ void a_wait_vm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
  }
}
constexpr int A_OOB = 0x7fffffff;
// sum over the 32 lanes of each wave half: quad and row rotations by DPP, one cross-row shuffle
__device__ __forceinline__ float a_dpp(float v, int ctl) {
  return __builtin_bit_cast(float, ctl == 0xB1 ? __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)
                                  : ctl == 0x4E ? __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)
                                  : ctl == 0x124 ? __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x124, 0xF, 0xF, true)
                                                 : __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));
}
__device__ __forceinline__ float a_sum32(float v) {
  v += a_dpp(v, 0xB1);   // quad_perm [1, 0, 3, 2]
  v += a_dpp(v, 0x4E);   // quad_perm [2, 3, 0, 1]
  v += a_dpp(v, 0x124);  // row_ror 4
  v += a_dpp(v, 0x128);  // row_ror 8
  return v + __shfl_xor(v, 16, 64);
}
}  // namespace

// MS: several KV streams (cross-attention); Q2: the Q/K/V stage-2 backward fused into the epilogue
// (AttnProblem::q2_*, self-attention only)
// DET (Q2 only; deterministic mode, mmt_det.h): a separate instantiation whose stage-2 epilogue stores the
// workgroup's dW2 / db1 sums as partials (partial index = batch element b) instead of adding them by atomics
// OC (Q2 only; AttnProblem::oc_*): Q / K / V are not read; the prologue makes the wave's K / V fragments and the
// Q slices of its two tiles from h1 and W2 (oc_tile), and only dO comes by LDS-DMA
template <bool DROP, bool MS, bool Q2, bool DET = false, bool OC = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_fused32(AttnBatch batch, int T, int H, float scale) {
  static_assert(!(MS && Q2), "the stage-2 backward follows the self-attention only");
  static_assert(!DET || Q2, "only the stage-2 epilogue has sums to store");
  static_assert(!OC || Q2, "on-chip Q/K/V goes with the stage-2 backward");
  constexpr int IMG = 8 * SL_SLICE;               // 256 rows x 32 columns as slice images
  constexpr int OFF_DO = IMG, OFF_TAB = 2 * IMG;  // tables: -LSE2 [256], -D (-D / sc under dropout) [256]
  constexpr int OFF_DS = OFF_TAB + 2048;          // per-wave [32][32] bf16 transpose slots
  constexpr int OFF_DQ = OFF_DS + 4 * 2048;       // dQ partials [2 steps][4 waves][32 q][32 d] fp32
  constexpr int BYTES = OFF_DQ + 8 * 4096;
  static_assert(2 * BYTES <= 160 * 1024, "two workgroups per CU");
  constexpr int EPW = 40;                          // epilogue transpose row stride (bf16)
  static_assert(4 * 32 * EPW * 2 <= 4 * 4096, "epilogue transposes alias one parity of the dQ partials");
  __shared__ __attribute__((aligned(1024))) char lds[BYTES];
  const AttnProblem& P = batch.p[blockIdx.z];
  const int nt = (T + 31) / 32;
  const int bh = xcd_tile(blockIdx.x, gridDim.x);
  const int b = bh / H, head = bh % H;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int64_t rowbase = (int64_t)b * T;
  const float c2 = scale * kLog2e;
  const int kts[2] = {w, 7 - w};
  // vector-memory operations a wave may leave in flight at step qt's barrier, behind its piece of slice
  // qt + 1: the pieces of slices qt + 2 .. nt - 1 and (not Q2: no dQ stores in the loop) the dQ stores of
  // steps 0 .. qt - 1
  auto in_flight = [&](int qt) { return Q2 ? nt - 2 - qt : nt - 2; };

  // Prologue. Every global load of the kernel is issued here and waited for (pinned) BEFORE the Q / dO
  // slices go out by LDS-DMA (the compiler counts only its own loads, so a wait it places while DMAs it
  // cannot see are in flight would drain them): the keep-bit words of the wave's (step, tile) slots, the
  // K / V rows of its key tiles, this thread's LSE / O / dO row. The slices then land while D, the
  // tables and K^T are built and while the first steps run: step qt waits (counted vmcnt) only for its
  // own piece of slice qt + 1, so the loop issues no other vector-memory operation but one dQ store per
  // step (a buffer store with out-of-range rows dropped: the count is fixed).
  // OC: in place of the K / V rows the loads are the h1 rows of the wave's two tiles (K, Q, V blocks: two 8-B
  // pieces per row and kind) and the head's three W2 blocks. Only dO goes out by DMA, from waves 1 and 3 as
  // before (nt pieces each, the same counted waits; waves 0 and 2 have no vector-memory operation in flight, so
  // their waits pass at once). While the pieces fly, every wave makes kf / vf of its key tiles and writes the Q
  // rows of its tiles w and 7 - w into the Q image (six MFMAs): the eight Q slices are all in LDS at the
  // prologue's barrier, ahead of step 0.
  const int64_t ntri = (int64_t)nt * (nt + 1) / 2;
  const int ns = MS ? P.nstreams : 1;
  // cross-attention (several KV streams): the workgroup walks the streams one after the other with Q / dO
  // resident; dQ sums over the streams in the caller's fp32 scratch rows (P.dq32: written by stream 0,
  // read-added by the middle streams, read and converted into dq by the last)
  const ai32x4 rdq32 = a_rsrc(MS ? P.dq32 + rowbase * P.dq32_ld + head * 32 : nullptr, MS ? (int64_t)T * P.dq32_ld * 4 : 0);
#pragma unroll 1
  for (int j = 0; j < ns; ++j) {
  const bf16_t* const oj = MS ? P.oj[j] : P.o;
  uint32_t mwq[2][8];  // keep-bit word of tile t at step q (key r; a FIFO shifted once per step)
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 8; ++q) {  // step q walks query tile q
      mwq[t][q] = 0u;
      if (DROP && q < nt && kts[t] <= q)
        mwq[t][q] = P.dmask[j][((int64_t)bh * ntri + q * (q + 1) / 2 + kts[t]) * 32 + key_dword(r)];
    }
  bf16x8 kf[2][2], vf[2][2];
  bf16x8 ocw[3], och[2][3];  // OC: W2 fragments of the K, Q, V blocks and the h1 fragments of the two tiles
  if constexpr (OC) {
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) {
      const int blk = kd * H + head;
      ocw[kd] = oc_w2frag(P.oc_w2, blk, r, h);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int tk = kts[t] * 32 + r;
        och[t][kd] = oc_hfrag(P.oc_h1 + (rowbase + tk) * P.oc_ld + blk * 16, h, tk < T);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 2 && !OC; ++t) {
    const int tk = kts[t] * 32 + r;
    const bool ok = kts[t] < nt && tk < T;
    const bf16_t* kp = P.k[j] + head * P.kv_hstride + (rowbase + tk) * P.kv_ld;
    const bf16_t* vp = P.v[j] + head * P.kv_hstride + (rowbase + tk) * P.kv_ld;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      kf[t][s] = ld8(kp + 16 * s + 8 * h, ok);
      vf[t][s] = ld8(vp + 16 * s + 8 * h, ok);
    }
  }
  float lse_t = 0.f;
  u32x4 ov[4], dv4[4];
  {
    const bool ok = tid < T;
    const int64_t t0 = ok ? tid : 0;
    lse_t = P.lse[j][(int64_t)bh * T + t0];
    const bf16_t* orow = oj + (rowbase + t0) * P.o_ld + head * 32;
    const bf16_t* drow = P.dout + (rowbase + t0) * P.dout_ld + head * 32;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ov[c] = *reinterpret_cast<const u32x4*>(orow + 8 * c);
      dv4[c] = *reinterpret_cast<const u32x4*>(drow + 8 * c);
    }
  }
  // Q2: W2^T of the head's K / Q / V stage-2 blocks as the A operand of dh1^T = W2^T dX^T (lane: i < 16,
  // k: o = 16 s + 8 h + 0..7; rows i >= 16 zero)
  // (one pinned base, unpredicated loads: lanes r >= 16 read row r - 16's words and drop them)
  bf16x8 w2t[3][2];
  const MMT_AS1 float* const w2p = Q2 ? sgpr_gptr(P.q2_w2) + head * 512 + (r & 15) + 8 * h * 16 : nullptr;
#pragma unroll
  for (int kd = 0; kd < 3; ++kd)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float wv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        wv[e] = Q2 ? w2p[(kd * H * 32 + 16 * s + e) * 16] : 0.f;
        wv[e] = r < 16 ? wv[e] : 0.f;
      }
      w2t[kd][s] = __builtin_bit_cast(bf16x8, u32x4{pack2bf(wv[0], wv[1]), pack2bf(wv[2], wv[3]), pack2bf(wv[4], wv[5]),
                                                   pack2bf(wv[6], wv[7])});
    }
  // pins: the compiler's waits for all of the above land here, ahead of the DMAs
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int q = 0; q < 8; ++q) asm volatile("" : "+v"(mwq[t][q]));
    if constexpr (OC) {
#pragma unroll
      for (int kd = 0; kd < 3; ++kd) asm volatile("" : "+v"(och[t][kd]));
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        asm volatile("" : "+v"(kf[t][s]));
        asm volatile("" : "+v"(vf[t][s]));
      }
    }
  }
  if constexpr (OC) {
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) asm volatile("" : "+v"(ocw[kd]));
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    asm volatile("" : "+v"(ov[c]));
    asm volatile("" : "+v"(dv4[c]));
  }
  asm volatile("" : "+v"(lse_t));
  if (Q2) {
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) {
      asm volatile("" : "+v"(w2t[kd][0]));
      asm volatile("" : "+v"(w2t[kd][1]));
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // Q (waves 0, 2) and dO (waves 1, 3) images: wave w streams column half w >> 1 of every slice, in
  // slice order (nt pieces: the loop's counted waits); once, for the first stream
  // (OC: the dO halves only, waves 1 and 3)
  if (j == 0 && (!OC || (w & 1))) {
    const int op = w & 1, cb = w >> 1;
    const int ld = op ? P.dout_ld : P.q_ld;
    const ai32x4 rs = a_rsrc((op ? P.dout : P.q) + rowbase * ld + head * 32, (int64_t)T * ld * 2);
    const int prow = lane >> 1, pcol = 8 * ((lane & 1) ^ ((prow >> 3) & 1));
    char* dst = lds + op * OFF_DO + cb * SL_SUB;
    for (int sl = 0; sl < nt; ++sl) {  // in step order
      const int grow = sl * 32 + prow;
      const int voff = grow < T ? (grow * ld + cb * 16 + pcol) * 2 : A_OOB;
      a_dma16(rs, __builtin_amdgcn_readfirstlane(a_lds_u32(dst + sl * SL_SLICE)), voff);
    }
  }
  if constexpr (OC) {
    // K / V fragments of the wave's key tiles and the Q rows of the same two tiles, into the Q image (piece pr
    // of lane (r, h) is chunk 2 pr + h of row r); tiles past nt come out as zeros and are never read
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      u32x4 x[2];
      oc_tile(ocw[0], och[t][0], x);
#pragma unroll
      for (int s = 0; s < 2; ++s) kf[t][s] = __builtin_bit_cast(bf16x8, x[s]);
      oc_tile(ocw[2], och[t][2], x);
#pragma unroll
      for (int s = 0; s < 2; ++s) vf[t][s] = __builtin_bit_cast(bf16x8, x[s]);
      oc_tile(ocw[1], och[t][1], x);
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) *reinterpret_cast<u32x4*>(lds + sl_off(kts[t] * 32 + r, 2 * pr + h)) = x[pr];
    }
  }
  // the LSE / D tables: thread t holds query t
  float* tab = reinterpret_cast<float*>(lds + OFF_TAB);
  {
    float dsum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dsum += bf2f(ov[c][e] & 0xffff) * bf2f(dv4[c][e] & 0xffff);
        dsum += bf2f(ov[c][e] >> 16) * bf2f(dv4[c][e] >> 16);
      }
    const bool ok = tid < T;
    tab[tid] = ok ? -lse_t : -INFINITY;  // rows past T: P = exp2(-inf) = 0 (the ragged last tile's mask)
    tab[256 + tid] = ok ? (DROP ? -dsum / P.drop_scale : -dsum) : 0.f;
  }
  // K^T of the wave's key tiles (d on lanes, keys in the permuted k order of the transposed reads),
  // through the wave's slot: the [key][q] dS image of the dQ product uses the same layout (8-B chunk c
  // of row k at chunk c ^ ((k >> 1) & 7)) and the same reads, so the two operands' k orders agree
  char* slot = lds + OFF_DS + w * 2048;
  const int g4 = lane >> 4, qq = (lane >> 2) & 3, p4 = lane & 3;
  const int ra0 = 4 * (g4 >> 1) + qq, ra1 = ra0 + 8;
  const int o_da0 = ra0 * 64 + (((4 * (g4 & 1) + p4) ^ ((ra0 >> 1) & 7)) << 3);
  const int o_da1 = ra1 * 64 + (((4 * (g4 & 1) + p4) ^ ((ra1 >> 1) & 7)) << 3);
  auto sw = [&](int c) { return r * 64 + ((c ^ ((r >> 1) & 7)) << 3); };  // 8-B chunk c of row r
  bf16x8 ktf[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const u32x4 v = __builtin_bit_cast(u32x4, kf[t][s]);
      *reinterpret_cast<u32x2*>(slot + sw(4 * s + 2 * h)) = u32x2{v[0], v[1]};
      *reinterpret_cast<u32x2*>(slot + sw(4 * s + 2 * h + 1)) = u32x2{v[2], v[3]};
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < 2; ++s) ktf[t][s] = join4(lds_tr16(slot + o_da0 + 1024 * s), lds_tr16(slot + o_da1 + 1024 * s));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  if (j == 0) a_wait_vm(nt - 1);  // this wave's piece of slice 0 (the younger nt - 1 pieces stay in flight)
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the previous stream's dQ-sum stores are done
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // everyone's slice-0 pieces and table entries (later streams: and every
                                 // wave is past the previous stream's epilogue)

  // element e of a tile accumulator is query row (e & 3) + 8 (e >> 2) + 4 h of the tile, key r: bit e
  // of m_diag keeps the diagonal tile's causal half. A ragged last query tile needs no mask of its own:
  // its rows past T have -inf LSE-table entries, and its keys past T lie above the diagonal
  uint32_t m_diag = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
    m_diag |= (uint32_t)(r <= row) << e;
  }
  const bf16_t* qimg = reinterpret_cast<const bf16_t*>(lds);
  const bf16_t* dimg = reinterpret_cast<const bf16_t*>(lds + OFF_DO);
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) { zero16(dk[t]); zero16(dv[t]); }

  // one owned key tile (t) against query tile qt; mw: the tile's keep bits (key r, this lane's half);
  // diag: the tile on the causal diagonal (kt == qt)
  auto tile = [&](int qt, int t, uint32_t mw, f32x16& dqp, bool diag) {
    asm volatile("" ::: "memory");  // the slot's previous reads stay ahead of this tile's writes
    const int q0 = qt * 32;
    bf16x8 qr[2], dr[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      qr[s] = sl_row(qimg, q0, r, s, h);
      dr[s] = sl_row(dimg, q0, r, s, h);
    }
    f32x16 sacc, dpacc;
    zero16(sacc);
    zero16(dpacc);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      sacc = mfma32(qr[s], kf[t][s], sacc);    // S[q][key]
      dpacc = mfma32(dr[s], vf[t][s], dpacc);  // dP[q][key]
    }
    if (diag) {  // wave-uniform: scores above the diagonal become -inf, touching only the score accumulator
      asm volatile("" ::: "memory");  // a real branch: selects on every tile cost 16 VALU
#pragma unroll
      for (int e = 0; e < 16; ++e) sacc[e] = (m_diag >> e) & 1 ? sacc[e] : -INFINITY;
    }
    uint32_t pp[8], dd[8];  // packed bf16 pairs of Z P (dV operand) and dS / sc (dK operand)
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(tab + q0 + 8 * gg + 4 * h);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(tab + 256 + q0 + 8 * gg + 4 * h);
#pragma unroll
      for (int e4 = 0; e4 < 4; e4 += 2) {
        float pm[2], ds[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int e = 4 * gg + e4 + u;
          const float pv = ex2(__builtin_fmaf(sacc[e], c2, l4[e4 + u]));
          if (DROP) {
            int kb = __builtin_amdgcn_sbfe((int)mw, 8 * gg + e4 + u, 1);  // all ones iff kept
            asm volatile("" : "+v"(kb));
            pm[u] = keep_f(pv, kb);
            ds[u] = __builtin_fmaf(pm[u], dpacc[e], pv * d4[e4 + u]);  // Z P dP - P D'
          } else {
            pm[u] = pv;
            ds[u] = pv * (dpacc[e] + d4[e4 + u]);  // P (dP - D)
          }
        }
        pp[2 * gg + e4 / 2] = pack2bf(pm[0], pm[1]);
        dd[2 * gg + e4 / 2] = pack2bf(ds[0], ds[1]);
      }
    }
    // dS -> the slot as [key][q] rows (lane (r, h): queries 8 gg + 4 h .. + 3 of key r)
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) *reinterpret_cast<u32x2*>(slot + sw(2 * gg + h)) = u32x2{dd[2 * gg], dd[2 * gg + 1]};
    bf16x8 dot[2], qtr[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      dot[s] = sl_tr(dimg, q0, s, lane);
      qtr[s] = sl_tr(qimg, q0, s, lane);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 pf = __builtin_bit_cast(bf16x8, u32x4{pp[4 * s], pp[4 * s + 1], pp[4 * s + 2], pp[4 * s + 3]});
      const bf16x8 df = __builtin_bit_cast(bf16x8, u32x4{dd[4 * s], dd[4 * s + 1], dd[4 * s + 2], dd[4 * s + 3]});
      dv[t] = mfma32(pf, dot[s], dv[t]);
      dk[t] = mfma32(df, qtr[s], dk[t]);
    }
    // dQ_w^T[d][q] += K^T[d][key] dS^T[key][q]: both fragments in the permuted k order of the slot reads
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 da = join4(lds_tr16(slot + o_da0 + 1024 * s), lds_tr16(slot + o_da1 + 1024 * s));
      dqp = mfma32(ktf[t][s], da, dqp);
    }
  };

  const float dqs = DROP ? scale * P.drop_scale : scale;
  const ai32x4 rdq = a_rsrc(P.dq + rowbase * P.dq_ld + head * 32, (int64_t)T * P.dq_ld * 2);
  const int R = 8 * w + (lane >> 3), cq = lane & 7;  // this wave's dQ rows / 16-B column chunk
  // The walk: all waves take query tile qt in step qt, one barrier per step. The diagonal tile's causal
  // mask is the only one (tile()); the dQ partials are double-buffered by step parity.
#pragma unroll 1
  for (int qt = 0; qt < nt; ++qt) {
    const uint32_t cA = mwq[0][0] >> (4 * h), cB = mwq[1][0] >> (4 * h);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 7; ++q) mwq[t][q] = mwq[t][q + 1];
    f32x16 dqp;
    zero16(dqp);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kt = kts[t];
      if (kt < nt && kt <= qt) tile(qt, t, t ? cB : cA, dqp, kt == qt);
    }
    char* part = lds + OFF_DQ + ((qt & 1) * 4 + w) * 4096;
    if (w <= qt) {  // this wave had a tile in the step (its key tile w is the lower one)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg)
        *reinterpret_cast<f32x4*>(part + r * 128 + (((2 * gg + h) ^ (r & 7)) << 4)) =
            f32x4{dqp[4 * gg], dqp[4 * gg + 1], dqp[4 * gg + 2], dqp[4 * gg + 3]};
    }
    if (j == 0 && qt + 1 < nt) a_wait_vm(in_flight(qt));  // this wave's piece of slice qt + 1
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every partial of step qt is written; slice qt + 1 landed
    {
      const int nw = min(qt + 1, 4);
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      for (int u = 0; u < nw; ++u)
        a += *reinterpret_cast<const f32x4*>(lds + OFF_DQ + ((qt & 1) * 4 + u) * 4096 + R * 128 + ((cq ^ (R & 7)) << 4));
      const int tq = qt * 32 + R;
      if (Q2) {  // dQ rows into the (spent) Q slice of this step, for the stage-2 backward after the walk
        *reinterpret_cast<u32x2*>(lds + qt * SL_SLICE + sl_off(R, cq >> 1) + (cq & 1) * 8) =
            u32x2{pack2bf(a[0] * dqs, a[1] * dqs), pack2bf(a[2] * dqs, a[3] * dqs)};
      } else if (!MS || j == ns - 1) {
        if (MS && j > 0 && tq < T) a += *reinterpret_cast<const f32x4*>(P.dq32 + (rowbase + tq) * P.dq32_ld + head * 32 + 4 * cq);
        a_bst8(rdq, tq < T ? (tq * P.dq_ld + 4 * cq) * 2 : A_OOB,
               u32x2{pack2bf(a[0] * dqs, a[1] * dqs), pack2bf(a[2] * dqs, a[3] * dqs)});
      } else {  // running fp32 sum over the streams (stream 0: one counted store per step, as above)
        if (j > 0 && tq < T) a += *reinterpret_cast<const f32x4*>(P.dq32 + (rowbase + tq) * P.dq32_ld + head * 32 + 4 * cq);
        a_bst16(rdq32, tq < T ? (tq * P.dq32_ld + 4 * cq) * 4 : A_OOB, a);
      }
    }
  }

  const float dks = DROP ? scale * P.drop_scale : scale;
  const float dvs = DROP ? P.drop_scale : 1.f;
  if constexpr (Q2) {
    // Q/K/V stage-2 backward of this head (model.py:36-50) on the 32-row tiles of dQ (in the Q image),
    // dK and dV (staged from the accumulators): per tile dh1^T = W2^T dX^T (2 MFMAs), times tanh' from
    // the tile's h1 rows, stored; dW2^T += dX^T h1 (2 MFMAs) and the dh1 column sums (db1) in registers
    // until the workgroup's sums go out by atomics. dQ / dK / dV never leave the kernel.
    // the h1 rows of the six tiles (key / query tiles kts[t] x K, Q, V blocks) in flight at once: the
    // tiles are worked one after the other, each wait only for its own rows
    u32x4 h1v[2][3];
    {
      const MMT_AS1 bf16_t* const h1 = sgpr_gptr(P.q2_h1);
      const int ld = __builtin_amdgcn_readfirstlane(P.q2_ld);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kd = 0; kd < 3; ++kd) {
          const int row = kts[t] * 32 + r;
          h1v[t][kd] = u32x4{0u, 0u, 0u, 0u};
          if (kts[t] < nt && row < T)
            h1v[t][kd] = *reinterpret_cast<const MMT_AS1 u32x4*>(h1 + (rowbase + row) * ld + (kd * H + head) * 16 + 8 * h);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's dQ rows of the last step are in the Q image
    char* xs = lds + OFF_DQ + w * SL_SLICE;              // this wave's dX tile (slice image)
    char* hs_ = lds + OFF_DQ + 4 * SL_SLICE + w * SL_SLICE;  // and its h1 tile (columns 16..31 zero)
    f32x16 dwa[3];
    float dba[3][8];
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) {
      zero16(dwa[kd]);
#pragma unroll
      for (int e = 0; e < 8; ++e) dba[kd][e] = 0.f;
    }
    MMT_AS1 bf16_t* const dh1 = sgpr_gptr(P.q2_dh1);
    const int ldd = __builtin_amdgcn_readfirstlane(P.q2_ld);
    auto tile_op = [&](int kd, const char* ximg, int row0, const u32x4& hv) {
      const int blk = kd * H + head;
      const int row = row0 + r;
      *reinterpret_cast<u32x4*>(hs_ + sl_off(r, h)) = hv;
      *reinterpret_cast<u32x4*>(hs_ + sl_off(r, 2 + h)) = u32x4{0u, 0u, 0u, 0u};
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      f32x16 acc;
      zero16(acc);
#pragma unroll
      for (int s = 0; s < 2; ++s)
        acc = mfma32(w2t[kd][s], sl_row(reinterpret_cast<const bf16_t*>(ximg), 0, r, s, h), acc);  // dh1^T[i][r]
      // lane (r, h): i = 4 h + e (e < 4) and 8 + 4 h + e - 4 (4 <= e < 8)
      const u32x2 ha = *reinterpret_cast<const u32x2*>(hs_ + sl_off(r, 0) + 8 * h);
      const u32x2 hb = *reinterpret_cast<const u32x2*>(hs_ + sl_off(r, 1) + 8 * h);
      float hh8[8] = {bf2f(ha[0] & 0xffff), bf2f(ha[0] >> 16), bf2f(ha[1] & 0xffff), bf2f(ha[1] >> 16),
                      bf2f(hb[0] & 0xffff), bf2f(hb[0] >> 16), bf2f(hb[1] & 0xffff), bf2f(hb[1] >> 16)};
      float d[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        d[e] = acc[e] * (1.f - hh8[e] * hh8[e]);
        dba[kd][e] += d[e];
      }
      if (row < T) {
        MMT_AS1 bf16_t* dst = dh1 + (rowbase + row) * ldd + blk * 16 + 4 * h;
        *reinterpret_cast<MMT_AS1 u32x2*>(dst) = u32x2{pack2bf(d[0], d[1]), pack2bf(d[2], d[3])};
        *reinterpret_cast<MMT_AS1 u32x2*>(dst + 8) = u32x2{pack2bf(d[4], d[5]), pack2bf(d[6], d[7])};
      }
      // dW2^T[i][o] ... as C[m = o][n = i]: A = dX^T (lane o), B = h1 (lane i), k = rows (permuted)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        dwa[kd] = mfma32(sl_tr(reinterpret_cast<const bf16_t*>(ximg), 0, s, lane),
                         sl_tr(reinterpret_cast<const bf16_t*>(hs_), 0, s, lane), dwa[kd]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this tile's LDS reads before the next writes
    };
    // dK, dV of the wave's key tiles: accumulators (lane: column o = r, elements: rows) -> the tile image
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kt = kts[t];
      if (kt >= nt) continue;
#pragma unroll
      for (int mtx = 0; mtx < 2; ++mtx) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int kr = (e & 3) + 8 * (e >> 2) + 4 * h;
          *reinterpret_cast<bf16_t*>(xs + sl_off(kr, r >> 3) + (r & 7) * 2) = mtx ? f2bf(dv[t][e] * dvs) : f2bf(dk[t][e] * dks);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        tile_op(mtx ? 2 : 0, xs, kt * 32, h1v[t][mtx ? 2 : 0]);
      }
    }
    // dQ tiles w and 7 - w from the Q image
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int qt = kts[t];
      if (qt < nt) tile_op(1, lds + qt * SL_SLICE, qt * 32, h1v[t][1]);
    }
    MMT_AS1 float* const db1 = sgpr_gptr(P.q2_db1);
    MMT_AS1 float* const dw2 = sgpr_gptr(P.q2_dw2);
    // db1: column sums over the 32 rows of each lane half; lane r < 24 of each half adds sum r
    {
      float mine = 0.f;
#pragma unroll
      for (int kd = 0; kd < 3; ++kd)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = a_sum32(dba[kd][e]);
          mine = r == kd * 8 + e ? v : mine;
        }
      const int kd = r >> 3, e = r & 7;
      if constexpr (DET) {
        // the wave's 48 sums into LDS behind the dW2 reduction area (past the tile images, which other waves
        // may still read: the dQ partials there are spent since the barrier above); summed over the waves below
        if (r < 24)
          reinterpret_cast<float*>(lds + OFF_DQ)[4 * 3 * 512 + w * 48 + kd * 16 + (e < 4 ? 4 * h + e : 8 + 4 * h + e - 4)] = mine;
      } else {
      if (r < 24)
        __hip_atomic_fetch_add(db1 + (kd * H + head) * 16 + (e < 4 ? 4 * h + e : 8 + 4 * h + e - 4), mine, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // dW2: the four waves' partials summed through LDS, one atomic per element
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's tile images are spent
    float* red = reinterpret_cast<float*>(lds + OFF_DQ);  // [4 waves][3 kinds][32 o][16 i]
    if (r < 16) {
#pragma unroll
      for (int kd = 0; kd < 3; ++kd)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          red[((w * 3 + kd) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h) * 16 + r] = dwa[kd][e];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (DET) {
      static_assert((4 * 3 * 512 + 4 * 48) * 4 <= 8 * 4096, "the reduction areas fit the dQ partials");
      const int nb = gridDim.x / H;  // batch elements = partials per element
      float* const dp = batch.det.base + (int64_t)blockIdx.z * batch.det.stride;
      for (int q = tid; q < 3 * 512; q += 256) {
        const float v = (red[q] + red[1536 + q]) + (red[3072 + q] + red[4608 + q]);
        const int kd = q / 512, oi = q % 512;
        dp[((int64_t)b * 3 * H + kd * H + head) * 512 + oi] = v;
      }
      if (tid < 48) {
        const float* dbw = red + 4 * 3 * 512;
        const float v = (dbw[tid] + dbw[48 + tid]) + (dbw[96 + tid] + dbw[144 + tid]);
        const int kd = tid / 16, col = tid % 16;
        dp[(int64_t)nb * 3 * H * 512 + ((int64_t)b * 3 * H + kd * H + head) * 16 + col] = v;
      }
      return;
    }
    for (int q = tid; q < 3 * 512; q += 256) {
      const float v = (red[q] + red[1536 + q]) + (red[3072 + q] + red[4608 + q]);
      const int kd = q / 512, oi = q % 512;
      __hip_atomic_fetch_add(dw2 + (kd * H + head) * 512 + oi, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  } else {
  // dK / dV of the wave's key tiles, transposed through LDS into row-major 16-B pieces (as the dK/dV
  // pass), one matrix at a time through the dQ partials of the parity the last step did not use (no
  // wave reads them after the last step's barrier; the next stream's first barrier retires these reads)
  bf16_t* et = reinterpret_cast<bf16_t*>(lds + OFF_DQ + (nt & 1) * 4 * 4096) + w * (32 * EPW);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int kt = kts[t];
    if (kt >= nt) continue;
    const int k0 = kt * 32;
#pragma unroll
    for (int mtx = 0; mtx < 2; ++mtx) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int kr = (e & 3) + 8 * (e >> 2) + 4 * h;
        et[kr * EPW + r] = mtx ? f2bf(dv[t][e] * dvs) : f2bf(dk[t][e] * dks);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      bf16_t* dst = (mtx ? P.dv[j] : P.dk[j]) + head * P.dkv_hstride;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = i * 16 + (lane >> 2), d0 = (lane & 3) * 8;
        const u32x4 v = *reinterpret_cast<const u32x4*>(et + row * EPW + d0);
        if (k0 + row < T) *reinterpret_cast<u32x4*>(dst + (rowbase + k0 + row) * P.dkv_ld + d0) = v;
      }
    }
  }
  }  // !Q2
  }  // streams
}

// =============================================================================================
// Host side: the knobs, the launch plan (mmt_attn_plan.h) and the launch switch. mmt_attn_plan and
// mmt_attn_mask_plan are the only places that decide an attention or mask launch.
// =============================================================================================
// Every knob of the attention dispatch, read once when the library loads. DESIGN.md section 3 has the table.
struct AttnKnobs {
  // MMT_ATTN_RING / mmt_attn_set_ring (in-process A/B): bit 0 the slice-streamed hs-64 dK/dV pass, bit 1 the
  // slice-streamed hs-64 dQ pass, bit 2 that dK/dV pass at 3 waves per SIMD (else 2), bit 3 the slice-streamed hs-64
  // forward, bit 4 unused, bit 5 the one-pass hs-64 backward at T <= 512 with one KV stream, bit 6 the one-pass
  // hs-32 backward at T <= 256, bit 7 that kernel also for several KV streams (with the fp32 dQ scratch)
  int ring = mmt_env_int("MMT_ATTN_RING", 15 | 64);
  // MMT_MASK_G: keep-bit tiles per wave of the mask kernel, 1, 2, 4, 8 or 16 (0: by T; another value: 8)
  int mask_g = mmt_env_int("MMT_MASK_G", 0);
  // mmt_attn_set_mask_g (no variable): the same, and ahead of MMT_MASK_G while it is not 0
  int mask_g_rt = 0;
};
static AttnKnobs g_ak;

extern "C" int mmt_attn_set_ring(int v) {
  const int old = g_ak.ring;
  g_ak.ring = v;
  return old;
}
extern "C" int mmt_attn_set_mask_g(int g) {
  const int old = g_ak.mask_g_rt;
  g_ak.mask_g_rt = g;
  return old;
}

int64_t mmt_attn_q2_det_floats(int count, int B, int H) { return (int64_t)count * B * 3 * H * (512 + 16); }

// the slice-streamed hs-64 kernels address a sequence's rows (and one (batch, head)'s keep-bit
// records) with 32-bit per-lane offsets from a per-batch-row buffer base: a sequence whose span
// reaches 2^31 bytes takes the chunked kernels (64-bit pointer math) instead
static bool ring64_fits(const AttnBatch& bt, int T) {
  const int64_t lim = (int64_t)1 << 31;
  const int64_t nt = (T + 31) / 32, ntri = nt * (nt + 1) / 2;
  if (ntri * 128 >= lim) return false;
  for (int g = 0; g < bt.count; ++g) {
    const AttnProblem& P = bt.p[g];
    if ((int64_t)T * P.q_ld * 2 >= lim || (int64_t)T * P.dout_ld * 2 >= lim || (int64_t)T * P.kv_ld * 2 >= lim)
      return false;
  }
  return true;
}

// the on-chip Q/K/V fields of one problem (AttnProblem::oc_*): 8-B row pieces of h1, 16-B rows of W2
static bool oc_ok(const AttnProblem& P) {
  return P.oc_h1 && P.oc_w2 && P.nstreams == 1 && !(P.oc_ld & 7) && !((uintptr_t)P.oc_h1 & 15) &&
         !((uintptr_t)P.oc_w2 & 15);
}

AttnPlan mmt_attn_plan(const AttnBatch& b, int B, int T, int H, int hs, bool bwd, int assume) {
  AttnPlan p{};
  p.status = ATTN_PLAN_EMPTY;
  if (b.count == 0 || B == 0 || T == 0) return p;
  p.status = ATTN_PLAN_INVALID;
  for (int g = 0; g < b.count; ++g) {
    if (b.p[g].nstreams < 1 || b.p[g].nstreams > MMT_MAX_STREAMS) return p;
    for (int j = 0; j < b.p[g].nstreams && b.p[g].nstreams > 1; ++j)  // per-stream outputs (summed, and
      if (!b.p[g].oj[j]) return p;                                      // read by the backward)
    if (b.p[g].drop_thr)  // dropout reads the keep bits of mmt_launch_attn_mask
      for (int j = 0; j < b.p[g].nstreams; ++j)
        if (!b.p[g].dmask[j]) return p;
    // one instantiation serves the whole batch, and the DROP one reads every problem's dmask: a batch that mixes
    // dropout on and off is refused
    if ((b.p[g].drop_thr != 0) != (b.p[0].drop_thr != 0)) return p;
  }
  for (int g = 0; g < b.count; ++g) {  // O / O_j leave the forward as 16-B row pieces
    if (b.p[g].o_ld & 7 || ((uintptr_t)b.p[g].o & 15)) return p;
    for (int j = 0; j < b.p[g].nstreams && b.p[g].nstreams > 1; ++j)
      if ((uintptr_t)b.p[g].oj[j] & 15) return p;
  }
  if (bwd) {  // all problems in a bwd batch must share nstreams (grid.x = tiles * B*H*nstreams)
    for (int g = 1; g < b.count; ++g)
      if (b.p[g].nstreams != b.p[0].nstreams) return p;
    // dQ, dK, dV leave the kernels as 16-B row pieces (8-element aligned rows and head offsets)
    for (int g = 0; g < b.count; ++g) {
      if ((b.p[g].dkv_ld & 7) || (b.p[g].dkv_hstride & 7)) return p;
      if ((b.p[g].dq_ld & 7) || ((uintptr_t)b.p[g].dq & 15)) return p;
      for (int j = 0; j < b.p[g].nstreams; ++j)
        if (((uintptr_t)b.p[g].dk[j] | (uintptr_t)b.p[g].dv[j]) & 15) return p;
    }
  }
  if (!attn_hs_built(hs)) return p;

  const int ring_kn = g_ak.ring;
  const bool drop = b.p[0].drop_thr != 0;
  const int nt = (T + 31) / 32, nb = (nt + 7) / 8, ns = b.p[0].nstreams;
  const auto set = [&](int i, int family, int gx) -> AttnLaunch& {
    AttnLaunch& l = p.l[i];
    l.family = family; l.hs = hs; l.drop = drop; l.gx = gx; l.gy = 1; l.gz = b.count; l.wg = 256;
    p.nlaunch = i + 1;
    return l;
  };
  // hs 64: the slice-streamed kernels (mmt_attn2.hip). Default: both backward passes on the rings (dQ: two query
  // tiles per wave), dK/dV at 3 waves per SIMD (standalone backward: target 277 -> 273 us, C3 cross-attention
  // 2461 -> 2298, C4 2237 -> 2116; C3 step -1.5 %: profiles/r3u_ring_ab.txt), and the forward on the ring too
  // (round 4: target 20.42 -> 20.34 ms, C3 157.3 -> 153.8 ms same box, profiles/r4m_ab.txt). MMT_ATTN_RING=0 keeps
  // the chunked ones.
  // ring depth 4 (three slices in flight): depth 6 measured slower (target backward 294 -> 301 us, C4
  // 2315 -> 2394 us: profiles/r3e_ring_slots_ab.txt); a one-query-tile-per-wave dQ ring equal at the
  // target and slower at C3, 8 key tiles per dK/dV workgroup slower at C3 / C4
  // (profiles/r3h_dkdv_waves_ab.txt), two plain dK/dV slices per barrier slower at C3 / C4
  // (profiles/r3u_ring_ab.txt): those variants were removed in round 4.
  const bool ring = hs == 64 && ring64_fits(b, T);
  if (!bwd) {
    bool oc = false;
    for (int g = 0; g < b.count; ++g) oc = oc || b.p[g].oc_w2 != nullptr;
    if (ring && (ring_kn & 8)) {  // knob bit 3: the forward on the LDS-DMA slice ring
      set(0, ATTN_RING64_FWD, nb * B * H).depth = 4;
    } else if (oc) {  // on-chip Q/K/V (AttnProblem::oc_*): hs 32, T <= 256, one stream, every problem; refused otherwise
      for (int g = 0; g < b.count; ++g)
        if (hs != 32 || T > 256 || !oc_ok(b.p[g])) return p;
      set(0, ATTN_OC32_FWD, B * H);
    } else {
      set(0, ATTN_CHUNK_FWD, nb * B * H);
    }
    p.status = ATTN_PLAN_OK;
    return p;
  }
  // The one-pass hs-32 backward (knob bit 6, round 6) takes the batch: T <= 256, Q / dO rows by LDS-DMA (16-B aligned
  // rows, sequences whose span fits a buffer descriptor); several KV streams only with knob bit 7 and the fp32 dQ
  // scratch. Every problem sets the Q/K/V stage-2 fields (AttnProblem::q2_*) or none does, and only with one KV
  // stream. Pointers count only as "field present" and by their alignment; ATTN_ASSUME_Q2 takes the stage-2 fields
  // as present and aligned.
  const bool a2 = (assume & ATTN_ASSUME_Q2) != 0;
  const bool q2 = a2 || b.p[0].q2_w2 != nullptr;
  const bool oc = b.p[0].oc_w2 != nullptr;
  bool f32 = hs == 32 && (ring_kn & 64) && T <= 256 && !(q2 && ns > 1);
  for (int g = 0; g < b.count && f32; ++g) {
    const AttnProblem& P = b.p[g];
    f32 = !(P.q_ld & 7) && !(P.dout_ld & 7) && !((uintptr_t)P.q & 15) && !((uintptr_t)P.dout & 15) && !(P.kv_ld & 7) &&
          !(P.kv_hstride & 7) && (int64_t)T * std::max(P.q_ld, P.dout_ld) * 2 < ((int64_t)1 << 31);
    // several KV streams (knob bit 7, off by default): one workgroup walks the streams in turn, and at
    // C1's cross-attention (3 streams, 512 workgroups: one generation) that measured slower than the
    // two-pass pair, which spreads the dK/dV pass over 3x the workgroups (70.7 vs 67.9 us standalone,
    // tools/attn_bench.py c1_ca)
    if (ns > 1)
      f32 = f32 && (ring_kn & 128) && P.dq32 && !(P.dq32_ld & 3) && !((uintptr_t)P.dq32 & 15) &&
            (int64_t)T * P.dq32_ld * 4 < ((int64_t)1 << 31);
    // one stream without the stage-2 fields: dQ rows leave as 8-B pieces
    if (ns == 1 && !q2) f32 = f32 && !(P.dq_ld & 3) && !((uintptr_t)P.dq & 7);
    if (!a2) {
      f32 = f32 && (P.q2_w2 != nullptr) == q2;
      if (q2)
        f32 = f32 && P.q2_h1 && P.q2_dh1 && P.q2_dw2 && P.q2_db1 && !(P.q2_ld & 7) && !((uintptr_t)P.q2_h1 & 15) &&
              !((uintptr_t)P.q2_dh1 & 7);
    }
    // on-chip Q/K/V: every problem or none, and only beside the stage-2 backward
    f32 = f32 && (P.oc_w2 != nullptr) == oc && (!oc || (q2 && oc_ok(P)));
  }
  // the stage-2 fields are a promise that the fused kernel writes dh1 / dW2 / db1 (and not dq / dk / dv):
  // refused rather than dropped when it cannot run (mmt_attn_bwd_fuses_qkv2 decides beforehand)
  for (int g = 0; g < b.count; ++g)
    if ((a2 || b.p[g].q2_w2 || b.p[g].oc_w2) && !f32) return p;
  p.status = ATTN_PLAN_OK;
  if (ring && (ring_kn & 32) && T <= 512 && ns == 1) {  // knob bit 5: dQ, dK, dV in one pass at hs 64
    set(0, ATTN_FUSED64, B * H).depth = 3;
  } else if (f32) {  // knob bit 6: dQ, dK, dV in one pass at hs 32
    AttnLaunch& l = set(0, ATTN_FUSED32, B * H);
    l.ms = ns > 1; l.q2 = q2; l.oc = oc;  // (oc: Q / K / V made in the prologue; only with q2)
    // deterministic mode: the stage-2 sums as per-batch-element partials, dW2 [B][3 H * 512] then db1
    // [B][3 H * 16] per problem, + the ordered sum
    l.det = q2 && b.det.base != nullptr;
    const int64_t stride = l.det ? mmt_attn_q2_det_floats(1, B, H) : 0;
    p.det_stride[0] = (int)(uint32_t)stride; p.det_stride[1] = (int)(stride >> 32);
  } else {
    // knob bit 1: the dQ pass on its ring; bit 0: the dK/dV pass, bit 2: at 3 waves per SIMD (<= 168 VGPRs)
    if (ring && (ring_kn & 2)) set(0, ATTN_RING64_DQ, nb * B * H).depth = 4;  // two query tiles per wave (8 per workgroup)
    else set(0, ATTN_CHUNK_DQ, nb * B * H);
    if (ring && (ring_kn & 1)) {
      AttnLaunch& l = set(1, ATTN_RING64_DKDV, ((nt + 3) / 4) * B * H * ns);
      l.occ = (ring_kn & 4) ? 3 : 2; l.depth = 4;
    } else {
      // dK/dV: one key tile per wave at 2 waves per SIMD (a paired two-key-tile walk at one wave per
      // SIMD measured slower: C1 103 vs 127 us, target step 25.4 vs 25.9 ms; removed in round 4)
      set(1, ATTN_CHUNK_DKDV, nb * B * H * ns);
    }
  }
  return p;
}

// launches one entry of the plan: the kernels of this file here, the others in their own translation units
static hipError_t launch_plan(const AttnBatch& bt, const AttnLaunch& l, int T, int H, float scale, hipStream_t s) {
  const dim3 grid(l.gx, l.gy, l.gz), wg(l.wg);
  switch (attn_key(l)) {
#define X(HS)                                                                                             \
  case attn_key(ATTN_CHUNK_FWD, HS, false): hipLaunchKernelGGL((attn_fwd_kernel<HS, false>), grid, wg, 0, s, bt, T, H, scale); break; \
  case attn_key(ATTN_CHUNK_FWD, HS, true): hipLaunchKernelGGL((attn_fwd_kernel<HS, true>), grid, wg, 0, s, bt, T, H, scale); break; \
  case attn_key(ATTN_CHUNK_DQ, HS, false): hipLaunchKernelGGL((attn_bwd_dq_kernel<HS, false>), grid, wg, 0, s, bt, T, H, scale); break; \
  case attn_key(ATTN_CHUNK_DQ, HS, true): hipLaunchKernelGGL((attn_bwd_dq_kernel<HS, true>), grid, wg, 0, s, bt, T, H, scale); break; \
  case attn_key(ATTN_CHUNK_DKDV, HS, false): hipLaunchKernelGGL((attn_bwd_dkdv1_kernel<HS, false>), grid, wg, 0, s, bt, T, H, scale); break; \
  case attn_key(ATTN_CHUNK_DKDV, HS, true): hipLaunchKernelGGL((attn_bwd_dkdv1_kernel<HS, true>), grid, wg, 0, s, bt, T, H, scale); break;
    ATTN_CHUNK_HS(X)
#undef X
#define X(D, MS, Q2, DET, OC)                                                                             \
  case attn_key(ATTN_FUSED32, 0, D, MS, Q2, DET, OC):                                                      \
    hipLaunchKernelGGL((attn_bwd_fused32<D, MS, Q2, DET, OC>), grid, wg, 0, s, bt, T, H, scale); break;
    ATTN_FUSED32_OPS(X)
#undef X
    default:
      if (l.family == ATTN_OC32_FWD) return mmt_attn_oc_launch_plan(bt, l, T, H, scale, s);
      return mmt_attn2_launch_plan(bt, l, T, H, scale, s);
  }
  return hipGetLastError();
}

static hipError_t attn_run(const AttnBatch& b, int B, int T, int H, int hs, float scale, bool bwd, hipStream_t s) {
  const AttnPlan p = mmt_attn_plan(b, B, T, H, hs, bwd);
  if (p.status != ATTN_PLAN_OK) return p.status == ATTN_PLAN_EMPTY ? hipSuccess : hipErrorInvalidValue;
  if (p.l[0].det) {  // the partials' region, the launch, then the ordered sums of every problem's dW2 and db1
    AttnBatch d = b;
    d.det.stride = attn_det_stride(p);
    DetLaunch L;
    hipError_t e = L.begin(d.det, d.count, d.det.stride, s);
    if (e == hipSuccess) e = launch_plan(d, p.l[0], T, H, scale, s);
    if (e != hipSuccess) return e;
    for (int g = 0; g < d.count; ++g) {
      L.seg(g, d.det.stride, 0, d.p[g].q2_dw2, B, 3 * H * 512);
      L.seg(g, d.det.stride, (int64_t)B * 3 * H * 512, d.p[g].q2_db1, B, 3 * H * 16);
    }
    return L.finish();
  }
  hipError_t e = hipSuccess;
  for (int i = 0; i < p.nlaunch && e == hipSuccess; ++i) e = launch_plan(b, p.l[i], T, H, scale, s);
  return e;
}

hipError_t mmt_launch_attn_fwd(const AttnBatch& b, int B, int T, int H, int hs, float scale, hipStream_t s) {
  return attn_run(b, B, T, H, hs, scale, false, s);
}
hipError_t mmt_launch_attn_bwd(const AttnBatch& b, int B, int T, int H, int hs, float scale, hipStream_t s) {
  return attn_run(b, B, T, H, hs, scale, true, s);
}

// =============================================================================================
// Dropout keep bits (AttnProblem::dmask): one wave per 32x32 (query tile, key tile <= query tile)
// tile of one (stream, bh). Lane (r, h) hashes query r's key pairs in the accumulator order of an
// S^T tile (one hash per key pair, mmt_keep on its 16-bit halves), and the ballot of each element
// is the element's two mask dwords. Pure VALU work with no inputs: launched on a side stream it
// overlaps the MFMA-bound GEMMs ahead of the attention.
// =============================================================================================
// A wave makes G consecutive tiles of the (stream, bh, row-major lower triangle) order: the index
// division, the triangle root and the row hash are paid once per wave (and per query tile) instead of
// once per tile.
// v_writelane_b32 (the LLVM intrinsic; hipcc exposes no builtin for it): a wave-uniform value into one lane
extern "C" __device__ int mmt_writelane(int v, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

template <int G>
__global__ __launch_bounds__(256) void attn_mask_kernel(AttnBatch batch, int BH, int T) {
  const AttnProblem& P = batch.p[blockIdx.z];
  const int nt = (T + 31) / 32;
  const int ntri = nt * (nt + 1) / 2;
  const int64_t per = (int64_t)BH * ntri;  // tiles per stream
  const int64_t total = per * P.nstreams;
  const int64_t t0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * G;
  if (P.drop_thr == 0 || t0 >= total) return;  // wave-uniform
  int j, bh, tri;
  int64_t tt;
  if (total <= 0x7fffffff) {  // 32-bit index arithmetic (an emulated 64-bit division costs ~150 instructions)
    const uint32_t t32 = (uint32_t)t0, p32 = (uint32_t)per;
    j = (int)(t32 / p32);
    const uint32_t r32 = t32 - (uint32_t)j * p32;
    bh = (int)(r32 / (uint32_t)ntri);
    tri = (int)(r32 - (uint32_t)bh * (uint32_t)ntri);
    tt = r32;
  } else {
    j = (int)(t0 / per);
    tt = t0 - (int64_t)j * per;
    bh = (int)(tt / ntri);
    tri = (int)(tt % ntri);
  }
  int qt = (int)((sqrtf(8.f * (float)tri + 1.f) - 1.f) * 0.5f);
  while (qt > 0 && qt * (qt + 1) / 2 > tri) --qt;
  while ((qt + 1) * (qt + 2) / 2 <= tri) ++qt;
  int kt = tri - qt * (qt + 1) / 2;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const uint32_t thr = P.drop_thr;
  uint32_t dkey = mmt_hash(P.drop_key, (uint32_t)j, MMT_STREAM_SALT);
  uint32_t rowh = mmt_prob_row(dkey, (uint32_t)(bh * T + qt * 32 + r));
  const int ng = (int)min<int64_t>(G, total - t0);
  for (int g = 0; g < ng; ++g) {
    // key pair c = kt*16 + 2h + off(e): the row hash plus the tile's part once, the pair offsets as constants
    const uint32_t hb = rowh + (uint32_t)(kt * 16 + 2 * h) * 0x9E3779B9u;
    uint32_t out = 0;   // lane L < 32: key-major dword L = half (L & 1) of element (L >> 1)'s ballot
    uint32_t word = 0;  // this lane's own 16 bits: element 2i at bit i, element 2i + 1 at bit 8 + i
#pragma unroll
    for (int e = 0; e < 16; e += 2) {  // keys k, k+1 (k even) share one hash
      const uint32_t off = (uint32_t)(((e & 3) >> 1) + 4 * (e >> 2));
      const uint32_t hk = mmt_prob_fin(hb + off * 0x9E3779B9u);
      const bool k0 = mmt_keep(hk, 0, thr), k1 = mmt_keep(hk, 1, thr);
      const uint64_t b0 = __builtin_amdgcn_ballot_w64(k0);
      const uint64_t b1 = __builtin_amdgcn_ballot_w64(k1);
      // the wave-uniform ballots straight into their lanes (elements e, e + 1 -> dwords 2e .. 2e + 3)
      out = (uint32_t)mmt_writelane((int)(uint32_t)b0, 2 * e, (int)out);
      out = (uint32_t)mmt_writelane((int)(uint32_t)(b0 >> 32), 2 * e + 1, (int)out);
      out = (uint32_t)mmt_writelane((int)(uint32_t)b1, 2 * e + 2, (int)out);
      out = (uint32_t)mmt_writelane((int)(uint32_t)(b1 >> 32), 2 * e + 3, (int)out);
      word |= (k0 ? 1u << (e >> 1) : 0u) | (k1 ? 1u << (8 + (e >> 1)) : 0u);  // (keep_spread, elem_keep)
    }
    uint32_t* const dm = P.dmask[j];
    if (lane < 32) dm[tt * 32 + lane] = out;
    reinterpret_cast<uint16_t*>(dm + (per + tt) * 32)[lane] = (uint16_t)word;
    // next tile: key tile, then query tile, then (b, h), then stream (wave-uniform branches)
    ++tt;
    if (++kt > qt) {
      kt = 0;
      if (++qt == nt) {
        qt = 0;
        if (++bh == BH) {
          bh = 0;
          tt = 0;
          ++j;
          dkey = mmt_hash(P.drop_key, (uint32_t)j, MMT_STREAM_SALT);
        }
      }
      rowh = mmt_prob_row(dkey, (uint32_t)(bh * T + qt * 32 + r));
    }
  }
}

AttnPlan mmt_attn_mask_plan(const AttnBatch& b, int B, int T, int H) {
  AttnPlan p{};
  p.status = ATTN_PLAN_EMPTY;
  if (b.count == 0 || B == 0 || T == 0) return p;
  p.status = ATTN_PLAN_INVALID;
  int ns = 0;
  for (int g = 0; g < b.count; ++g) {
    const AttnProblem& P = b.p[g];
    if (!P.drop_thr) continue;
    if (P.nstreams < 1 || P.nstreams > MMT_MAX_STREAMS) return p;
    for (int j = 0; j < P.nstreams; ++j)
      if (!P.dmask[j]) return p;
    ns = P.nstreams > ns ? P.nstreams : ns;
  }
  if (ns == 0) {  // no problem drops
    p.status = ATTN_PLAN_EMPTY;
    return p;
  }
  const int64_t tiles = mmt_attn_mask_tiles(B, H, T) * ns;
  // tiles per wave, by default:
  // (16 against 8 at T = 1024 / 4096: C3 140.3-140.4 -> 139.3-140.0 ms, C4 319.4-319.5 -> 317.6-318.7; at C1
  // (T = 256) equal within noise, so 8 below T = 1024: profiles/r6aq_mask_g16_ab.txt)
  // (8 against 4: C3 142.3 -> 140.9-141.1 ms, C1 / target equal; 4 against 1, the one-tile form: C3 149.2 ->
  // 143.7, target 19.40 -> 19.24, C1 7.98 -> 7.91: profiles/r6aa_mask_pileup.txt, r6ab_mask_ab.txt)
  const int gv = g_ak.mask_g_rt ? g_ak.mask_g_rt : g_ak.mask_g ? g_ak.mask_g : T >= 1024 ? 16 : 8;
  AttnLaunch& l = p.l[0];
  l.family = ATTN_MASK;
  l.g = (gv == 1 || gv == 2 || gv == 4 || gv == 16) ? gv : 8;
  const int64_t waves = (tiles + l.g - 1) / l.g;
  l.gx = (int)(unsigned)((waves + 3) / 4); l.gy = 1; l.gz = b.count; l.wg = 256;
  p.nlaunch = 1;
  p.status = ATTN_PLAN_OK;
  return p;
}

hipError_t mmt_launch_attn_mask(const AttnBatch& b, int B, int T, int H, hipStream_t s) {
  const AttnPlan p = mmt_attn_mask_plan(b, B, T, H);
  if (p.status != ATTN_PLAN_OK) return p.status == ATTN_PLAN_EMPTY ? hipSuccess : hipErrorInvalidValue;
  const AttnLaunch& l = p.l[0];
  const dim3 grid((unsigned)l.gx, l.gy, l.gz), wg(l.wg);
  switch (attn_key(l)) {
#define X(G) \
  case attn_key(ATTN_MASK, G, false): hipLaunchKernelGGL(attn_mask_kernel<G>, grid, wg, 0, s, b, B * H, T); break;
    ATTN_MASK_G(X)
#undef X
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
