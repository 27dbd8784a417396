// Device-side pieces shared by the attention translation units (mmt_attn.hip, mmt_attn_oc.hip): tile geometry,
// LDS slice images, chunk and keep-bit stagers, the forward's online softmax and step, and the on-chip Q/K/V
// stage-2 helpers (AttnProblem::oc_*). Everything here has internal linkage or is inlined.
#pragma once
#include <stdlib.h>

#include <algorithm>

#include <type_traits>

#include "mmt_common.h"
#include "mmt_kernels.h"

namespace {

__device__ __forceinline__ bf16x8 zero8() {
  const u32x4 z = {0u, 0u, 0u, 0u};
  return __builtin_bit_cast(bf16x8, z);
}

__device__ __forceinline__ bf16x8 ld8(const bf16_t* p, bool ok) {
  if (!ok) return zero8();
  return *reinterpret_cast<const bf16x8*>(p);
}

template <int HS>
struct Geo {
  static constexpr int NKS = (HS + 15) / 16;           // k-steps over the head dim
  static constexpr int ND = (HS + 31) / 32;            // 32-wide output tiles over the head dim
  static constexpr int W = ND * 32;                    // padded head width in LDS tiles
  static constexpr int RW = W + 8;                     // row-read tile stride (16-B pad: no b128 conflicts)
  static constexpr int TW = (W == 64) ? 96 : W;        // transposed-read tile stride (conflict-free)
  static constexpr int CH = HS / 8;                    // 16-byte chunks per row
};

// one 16-B chunk (8 bf16) of a 32-row tile: row r0+row, columns col..col+7 of the head (zero padded)
__device__ __forceinline__ u32x4 tile_chunk(const bf16_t* base, int64_t rowbase, int r0, int row, int col, int T,
                                            int ld) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (r0 + row < T) v = *reinterpret_cast<const u32x4*>(base + (rowbase + r0 + row) * ld + col);
  return v;
}

// A-operand fragment of X^T where X is a [32 rows][stride] LDS tile: lane gets column
// d = dt*32 + (lane&31) and rows {16s+4h+0..3, 16s+8+4h+0..3} (the accumulator-as-operand k order)
__device__ __forceinline__ bf16x8 tr_frag(const bf16_t* lds, int stride, int dt, int s, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const int q = i >> 2, p = i & 3;
  const int col = dt * 32 + 16 * (g & 1) + 4 * p;
  const int kb = 16 * s + 4 * (g >> 1) + q;
  return join4(lds_tr16(lds + kb * stride + col), lds_tr16(lds + (kb + 8) * stride + col));
}

// hs-32 slice image of the backward's shared operands (round 5, as the hs-64 rings' images of
// mmt_attn2.hip): 32-row slices of two 16-column sub-images 1152 B apart (1 KiB + 128 B pad), the two
// 16-B halves of a row swapped when bit 3 of the row is set. Row reads (ds_read_b128, a row per lane)
// and transposed reads (ds_read_b64_tr_b16, 4 rows x 16 columns per 16-lane group) are both
// conflict-free; the [row][40] image of Geo<32>::RW took 2-way conflicts on every transposed read
// (SQ_LDS_BANK_CONFLICT 0.31 / 0.25 of the dQ / dK-dV passes' LDS cycles at C1, round 4)
constexpr int SL_SUB = 1152, SL_SLICE = 2 * SL_SUB;
template <int HS>
struct SliceImg {
  static constexpr bool on = HS == 32;
};
// byte offset of 16-B chunk `chunk` (8 columns, 0..3) of row `row`
__device__ __forceinline__ int sl_off(int row, int chunk) {
  return (row >> 5) * SL_SLICE + (chunk >> 1) * SL_SUB + (row & 31) * 32 + (((chunk & 1) ^ ((row >> 3) & 1)) << 4);
}
// row fragment: row row0 + r of the slice at row0 (a multiple of 32), columns 16 s + 8 h .. + 7
// (per-lane part r 32 + swapped half: one register; the slice and s are immediates / scalars)
__device__ __forceinline__ bf16x8 sl_row(const bf16_t* img, int row0, int r, int s, int h) {
  const int o = (row0 >> 5) * SL_SLICE + s * SL_SUB + r * 32 + ((h ^ ((r >> 3) & 1)) << 4);
  return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(img) + o);
}
// transposed fragment of the slice at row0 (as tr_frag: column 16 (g & 1) + 4 p of rows
// 16 s + 4 (g >> 1) + q and + 8): the first row set has bit 3 clear, the second set, so the swap is
// fixed per set and the per-lane parts are two registers
__device__ __forceinline__ bf16x8 sl_tr(const bf16_t* img, int row0, int s, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int L = (g & 1) * SL_SUB + (p & 1) * 8 + (4 * (g >> 1) + q) * 32;
  const char* b = reinterpret_cast<const char*>(img) + (row0 >> 5) * SL_SLICE + 512 * s;
  return join4(lds_tr16(b + L + ((p >> 1) << 4)), lds_tr16(b + L + 256 + (((p >> 1) ^ 1) << 4)));
}

// accumulator registers 8s..8s+7 -> bf16 operand fragment
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& a, int s) {
  const u32x4 v = {pack2bf(a[8 * s], a[8 * s + 1]), pack2bf(a[8 * s + 2], a[8 * s + 3]),
                   pack2bf(a[8 * s + 4], a[8 * s + 5]), pack2bf(a[8 * s + 6], a[8 * s + 7])};
  return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ void zero16(f32x16& a) {
#pragma unroll
  for (int e = 0; e < 16; ++e) a[e] = 0.f;
}

__device__ __forceinline__ float keep_f(float v, int m) { return __int_as_float(__float_as_int(v) & m); }

// dword of an S^T mask tile that holds key r's keep bits over the tile's 32 queries
__device__ __forceinline__ int key_dword(int r) { return 2 * ((r & 3) + 4 * (r >> 3)) + ((r >> 2) & 1); }

// On-chip Q/K/V stage 2 at hs 32 (AttnProblem::oc_*): one 32-row tile of one kind is ONE K = 16 MFMA
// X^T[o][row] = W2[o][k] h1^T[k][row] with the operand roles, the K-slot order (lane (r, h), slot j <->
// k = 4 h + j for j < 4, 8 + 4 h + j - 4 for j >= 4), the zero accumulator and the bf16 packing of the
// stage-1 GEMM's fused epilogue (qkv2_fused, mmt_gemm.hip): the same bits as the rows that kernel stores.
// A operand: block blk of W2 (fp32 [32][16]) converted as qkv2_stage_w2 does, lane (o = r, h)
__device__ __forceinline__ bf16x8 oc_w2frag(const float* w2, int blk, int r, int h) {
  const float* w = w2 + ((int64_t)blk * 32 + r) * 16 + 4 * h;
  const f32x4 lo = *reinterpret_cast<const f32x4*>(w);
  const f32x4 hi = *reinterpret_cast<const f32x4*>(w + 8);
  return __builtin_bit_cast(bf16x8, u32x4{pack2bf(lo[0], lo[1]), pack2bf(lo[2], lo[3]), pack2bf(hi[0], hi[1]),
                                          pack2bf(hi[2], hi[3])});
}
// B operand: the 16 h1 columns at p (this lane's row, the block's first column), two 8-B pieces; !ok: zeros
__device__ __forceinline__ bf16x8 oc_hfrag(const bf16_t* p, int h, bool ok) {
  u32x2 a = {0u, 0u}, b = {0u, 0u};
  if (ok) {
    a = *reinterpret_cast<const u32x2*>(p + 4 * h);
    b = *reinterpret_cast<const u32x2*>(p + 8 + 4 * h);
  }
  return __builtin_bit_cast(bf16x8, u32x4{a[0], a[1], b[0], b[1]});
}
// the product, as 16-B row pieces after the v_permlane32_swap pairing of qkv2_fused's put: out[pr] = row r,
// columns 16 pr + 8 h .. + 7 (chunk 2 pr + h of the row; also the (r, h) operand fragment of k-step pr)
__device__ __forceinline__ void oc_tile(bf16x8 w2f, bf16x8 hf, u32x4 (&out)[2]) {
  f32x16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  const f32x16 d = mfma32(w2f, hf, z);
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    const int ga = 2 * pr, gb = 2 * pr + 1;
    const auto s0 = __builtin_amdgcn_permlane32_swap(pack2bf(d[4 * ga], d[4 * ga + 1]), pack2bf(d[4 * gb], d[4 * gb + 1]),
                                                     false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(pack2bf(d[4 * ga + 2], d[4 * ga + 3]),
                                                     pack2bf(d[4 * gb + 2], d[4 * gb + 3]), false, false);
    out[pr] = u32x4{s0[0], s1[0], s0[1], s1[1]};
  }
}

}  // namespace

// =============================================================================================
// Chunked staging. A workgroup (4 waves) owns 8 consecutive 32-row tiles of one (batch, head);
// wave w takes tiles w and 7-w, so the causal work of the 4 waves is balanced. The operand the
// tiles share (K/V in the forward and dQ pass, Q/dO in the dK/dV pass) is staged into LDS in
// chunks of ROWS rows (32 KiB of bf16 per operand pair): at T <= ROWS the whole sequence lands with
// one barrier and the waves then run barrier-free; longer sequences reload between chunks (the
// other resident workgroups of the CU cover that latency; a register prefetch would cost the
// occupancy it buys). Softmax runs in the log2 domain (scale * log2(e) folded into
// one multiply, exp2 on v_exp_f32); only tiles on the causal diagonal (and a ragged last query
// tile) evaluate the mask.
// =============================================================================================
template <int HS>
struct Chunk {
  static constexpr int ROWS = (HS <= 32) ? 256 : 128;
  static constexpr int HALF = ROWS * Geo<HS>::CH;  // 16-B pieces of one operand
  static constexpr int NSTG = 2 * HALF / 256;      // pieces per thread (two operands)
};

template <int HS>
struct Stager {
  u32x4 v[Chunk<HS>::NSTG];
  // rows [r0, r0 + ROWS) of operands a, b (columns 0..HS-1); rows >= T read as zeros
  __device__ __forceinline__ void load(const bf16_t* a, int lda, const bf16_t* b, int ldb, int64_t rowbase, int r0,
                                       int T, int tid) {
    constexpr int CH = Geo<HS>::CH, HALF = Chunk<HS>::HALF;
#pragma unroll
    for (int u = 0; u < Chunk<HS>::NSTG; ++u) {
      const int c = tid + 256 * u;
      const bool isb = c >= HALF;
      const int cc = isb ? c - HALF : c;
      v[u] = tile_chunk(isb ? b : a, rowbase, r0, cc / CH, (cc % CH) * 8, T, isb ? ldb : lda);
    }
  }
  // operand a's chunks only (a second image of it at another stride)
  __device__ __forceinline__ void store_a(bf16_t* la, int sa, int tid) const {
    constexpr int CH = Geo<HS>::CH, HALF = Chunk<HS>::HALF;
#pragma unroll
    for (int u = 0; u < Chunk<HS>::NSTG; ++u) {
      const int c = tid + 256 * u;
      if (c < HALF) *reinterpret_cast<u32x4*>(la + (c / CH) * sa + (c % CH) * 8) = v[u];
    }
  }
  __device__ __forceinline__ void store(bf16_t* la, int sa, bf16_t* lb, int sb, int tid) const {
    constexpr int CH = Geo<HS>::CH, HALF = Chunk<HS>::HALF;
#pragma unroll
    for (int u = 0; u < Chunk<HS>::NSTG; ++u) {
      const int c = tid + 256 * u;
      const bool isb = c >= HALF;
      const int cc = isb ? c - HALF : c;
      const int row = cc / CH, col = (cc % CH) * 8;
      *reinterpret_cast<u32x4*>(isb ? lb + row * sb + col : la + row * sa + col) = v[u];
    }
  }
  // both operands as slice images (SliceImg; HS == 32: 4 chunks per row)
  __device__ __forceinline__ void store_slices(bf16_t* la, bf16_t* lb, int tid) const {
    constexpr int CH = Geo<HS>::CH, HALF = Chunk<HS>::HALF;
    static_assert(CH == 4, "slice images hold 32 columns");
#pragma unroll
    for (int u = 0; u < Chunk<HS>::NSTG; ++u) {
      const int c = tid + 256 * u;
      const bool isb = c >= HALF;
      const int cc = isb ? c - HALF : c;
      *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(isb ? lb : la) + sl_off(cc / CH, cc % CH)) = v[u];
    }
  }
};

// Dropout keep bits of one staged chunk: LDS [8 block tiles][KT chunk tiles][32 dwords]. The block
// tiles are the block's 8 query tiles (forward, dQ) or key tiles (dK/dV); the chunk tiles are the
// key (query) tiles of the staged chunk. Tiles above the causal diagonal are left as zeros.
template <int HS, int KT_ = Chunk<HS>::ROWS / 32>
struct MaskStager {
  static constexpr int KT = KT_;
  static constexpr int N4 = 8 * KT * 8;  // 16-B pieces
  static constexpr int PER = (N4 + 255) / 256;
  static constexpr int DWORDS = 8 * KT * 32;
  u32x4 v[PER];
  // b0: first block tile, c0: first chunk tile; blk_q: block tiles are query tiles
  __device__ __forceinline__ void load(const uint32_t* base, int bh, int nt, int b0, int c0, bool blk_q, int tid) {
    const int64_t ntri = (int64_t)nt * (nt + 1) / 2;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int c = tid + 256 * u;
      v[u] = u32x4{0u, 0u, 0u, 0u};
      if (N4 % 256 == 0 || c < N4) {
        const int i = c / (KT * 8), k = (c / 8) % KT, p = c % 8;
        const int qt = blk_q ? b0 + i : c0 + k, kt = blk_q ? c0 + k : b0 + i;
        if (qt < nt && kt <= qt)
          v[u] = *reinterpret_cast<const u32x4*>(base + ((int64_t)bh * ntri + qt * (qt + 1) / 2 + kt) * 32 + p * 4);
      }
    }
  }
  __device__ __forceinline__ void store(uint32_t* lds, int tid) const {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int c = tid + 256 * u;
      if (N4 % 256 == 0 || c < N4) *reinterpret_cast<u32x4*>(lds + 4 * c) = v[u];
    }
  }
};

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// Softmax / dS arithmetic is scalar fp32 on purpose: v_pk_*_f32 beside MFMAs costs more issue
// cycles than the two scalar instructions it replaces (MI355X_MICROARCH.md, constants table), and
// this file is compiled with -fno-slp-vectorize so the compiler does not re-pack them.

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kTau = 8.0f;  // lazy-rescale threshold of the forward's running max (log2 units)

// waves per SIMD the forward / dQ kernels are compiled for (hs <= 32 fits two at no spill; at hs
// = 64 the forward fits two without AGPRs; the dQ pass spills ~25 VGPRs there and is still faster)
#ifndef MMT_FWD_MINB
#define MMT_FWD_MINB(hs) 2
#endif
#ifndef MMT_DQ_MINB
#define MMT_DQ_MINB(hs) 2
#endif
// single-tile dK/dV: at hs <= 32 the default bound (the compiler keeps the accumulators in AGPRs
// and still reaches 2 waves) measured faster than forcing 2; at hs = 64 forcing 2 fits without AGPRs
#ifndef MMT_DKDV1_MINB
#define MMT_DKDV1_MINB(hs) ((hs) <= 32 ? 1 : 2)
#endif

// cross-half reductions (lanes l and l ^ 32) in one v_permlane32_swap: no LDS round trip
__device__ __forceinline__ float xhalf_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  float m;
  asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(__uint_as_float(r[0])), "v"(__uint_as_float(r[1])));
  return m;
}
__device__ __forceinline__ float xhalf_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// Lane word of an S^T keep tile (attn_mask_kernel): bit i = element 2i, bit 8 + i = element 2i + 1
// of the lane's 16 accumulator elements. keep_spread moves the odd byte to bits 16..23 (one
// v_perm_b32); pair_keep then turns pair i (the two elements one v_cvt_pk_bf16_f32 packs) into a
// 0x0000 / 0xFFFF half mask with one shift and one packed arithmetic shift: 1.5 VALU per element
// including the AND on the packed bf16 pair.
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t keep_spread(uint32_t w16) { return __builtin_amdgcn_perm(0u, w16, 0x0c010c00u); }
__device__ __forceinline__ uint32_t pair_keep(uint32_t w32, int i) {
  s16x2 v = __builtin_bit_cast(s16x2, w32 << (15 - i));
  v = v >> (s16x2){15, 15};
  return __builtin_bit_cast(uint32_t, v);
}
// keep mask (all ones / zero) of element e of a lane word (fp32 selects in the dQ pass)
__device__ __forceinline__ int elem_keep(uint32_t w16, int e) {
  return __builtin_amdgcn_sbfe((int)w16, (e & 1) * 8 + (e >> 1), 1);
}

// accumulator registers 8s..8s+7 -> bf16 operand fragment, dropped elements zeroed
__device__ __forceinline__ bf16x8 acc_frag_keep(const f32x16& a, int s, uint32_t w32) {
  const u32x4 v = {pack2bf(a[8 * s], a[8 * s + 1]) & pair_keep(w32, 4 * s),
                   pack2bf(a[8 * s + 2], a[8 * s + 3]) & pair_keep(w32, 4 * s + 1),
                   pack2bf(a[8 * s + 4], a[8 * s + 5]) & pair_keep(w32, 4 * s + 2),
                   pack2bf(a[8 * s + 6], a[8 * s + 7]) & pair_keep(w32, 4 * s + 3)};
  return __builtin_bit_cast(bf16x8, v);
}

// per query tile state of the forward walk: Q fragments, running max / sum, O^T accumulators.
// l is this lane's HALF of the row sum (keys 4h + ..., combined across halves at the end): the
// two halves always share m (the max is reduced across them every tile)
template <int HS>
struct FwdQ {
  bf16x8 qf[Geo<HS>::NKS];
  f32x16 o[Geo<HS>::ND];
  float m, l;
  int tq;
};

// online softmax of one S^T tile for one query tile (log2 domain, lazy rescale)
template <int HS, bool diag>
__device__ __forceinline__ void fwd_softmax(f32x16& sacc, FwdQ<HS>& q, int k0, float c2, int h) {
  using G = Geo<HS>;
  // row max on the raw scores (c2 > 0 commutes with max), then into the log2 domain
  float tmax = -INFINITY;
  if (diag) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (key > q.tq) sacc[e] = -INFINITY;
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) tmax = fmaxf(tmax, sacc[e]);
  tmax = xhalf_max(tmax) * c2;
  // lazy rescale: the running max m moves only when a tile's max exceeds it by more than kTau
  // (log2 units; always on the first tile, m = -inf). Until then exp2(s - m) <= 2^kTau keeps P, l
  // and O comfortably in fp32/bf16 range and the O accumulators are not touched on the common
  // path. l and O share m, so the normalised output and the LSE m + log2(l) are unchanged.
  const bool up = tmax > q.m + kTau;
  if (__builtin_amdgcn_ballot_w64(up)) {  // wave-uniform
    const float alpha = up ? ex2(q.m - tmax) : 1.f;
    q.m = up ? tmax : q.m;
    q.l *= alpha;
#pragma unroll
    for (int dt = 0; dt < G::ND; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) q.o[dt][e] *= alpha;
  }
  const float nm = -q.m;
#pragma unroll
  for (int e = 0; e < 16; ++e) sacc[e] = ex2(__builtin_fmaf(sacc[e], c2, nm));
  // the row sum keeps every term (dropout acts on the normalised probabilities); four partial
  // chains, no cross-half reduction per tile
  float r0 = sacc[0] + sacc[1], r1 = sacc[2] + sacc[3], r2 = sacc[4] + sacc[5], r3 = sacc[6] + sacc[7];
  r0 += sacc[8] + sacc[9]; r1 += sacc[10] + sacc[11]; r2 += sacc[12] + sacc[13]; r3 += sacc[14] + sacc[15];
  q.l += (r0 + r1) + (r2 + r3);
}

// forward step over one 32-key tile for one or two query tiles (NQ): the K fragments and the
// transposed V fragments are read from LDS once and feed both tiles' MFMAs; the V reads are
// issued before the softmax so their latency hides under it
template <int HS, int NQ, bool DA, bool DB, bool DROP>
__device__ __forceinline__ void fwd_step(const bf16_t* ks, const bf16_t* vs, int kl, int k0, FwdQ<HS>& a, FwdQ<HS>& b,
                                         const uint32_t* mta, const uint32_t* mtb, float c2, int lane) {
  using G = Geo<HS>;
  const int r = lane & 31, h = lane >> 5;
  const uint32_t wa = DROP ? keep_spread(reinterpret_cast<const uint16_t*>(mta)[lane]) : 0u;
  const uint32_t wb = (DROP && NQ == 2) ? keep_spread(reinterpret_cast<const uint16_t*>(mtb)[lane]) : 0u;
  f32x16 sa, sb;
  zero16(sa);
  if (NQ == 2) zero16(sb);
#pragma unroll
  for (int s = 0; s < G::NKS; ++s) {
    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ks + (kl + r) * G::RW + 16 * s + 8 * h);
    sa = mfma32(kf, a.qf[s], sa);
    if (NQ == 2) sb = mfma32(kf, b.qf[s], sb);
  }
  bf16x8 vf[2][G::ND];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int dt = 0; dt < G::ND; ++dt) vf[s][dt] = tr_frag(vs + kl * G::TW, G::TW, dt, s, lane);
  fwd_softmax<HS, DA>(sa, a, k0, c2, h);
  if (NQ == 2) fwd_softmax<HS, DB>(sb, b, k0, c2, h);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x8 pa = DROP ? acc_frag_keep(sa, s, wa) : acc_frag(sa, s);
#pragma unroll
    for (int dt = 0; dt < G::ND; ++dt) a.o[dt] = mfma32(vf[s][dt], pa, a.o[dt]);
    if (NQ == 2) {
      const bf16x8 pb = DROP ? acc_frag_keep(sb, s, wb) : acc_frag(sb, s);
#pragma unroll
      for (int dt = 0; dt < G::ND; ++dt) b.o[dt] = mfma32(vf[s][dt], pb, b.o[dt]);
    }
  }
}
