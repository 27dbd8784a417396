// The sampler's device code (mmt.h: mmt_sample), shared by mmt_sample.hip (the draw, the score of a given token) and
// mmt_forecast.hip (the law a row's token is drawn from): the reductions, the weight of an element, the threshold
// search of top-k / top-p and the sums in vocabulary order. One definition, so the three agree bit for bit on a
// row's maximum m, threshold key K and normaliser S. Everything here assumes a 256-thread workgroup on one row.
#pragma once
#include "mmt_common.h"

namespace {

constexpr int SAMPLE_THREADS = 256;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / MMT_WAVE;
constexpr int SAMPLE_ONCHIP = 8192;      // largest V whose row lives in LDS
constexpr int SAMPLE_MAX_V = 1 << 20;    // largest V of the strided path

// order-preserving key: a < b (floats, no NaN) <=> okey(a) < okey(b)
__device__ __forceinline__ uint32_t okey(float z) {
  const uint32_t b = __float_as_uint(z);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct SampleShared {
  float f[2][SAMPLE_WAVES];
  double d[2][3][SAMPLE_WAVES];
  unsigned long long q[2][SAMPLE_WAVES];
  int i[2][SAMPLE_WAVES];
  int j[2][SAMPLE_WAVES];
};

// block reductions: wave butterfly (every lane ends with the same value), the four wave results combined left to
// right by every thread. The slots are double buffered by `par`, so one barrier per reduction suffices: a slot is
// rewritten two reductions later, after a barrier every reader has passed.
// three sums at once (the three candidates of one search round): independent chains, one barrier
__device__ __forceinline__ void block_sum3(double (&v)[3], SampleShared& sh, int& par) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] += __shfl_xor(v[k], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) sh.d[par][k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = ((sh.d[par][k][0] + sh.d[par][k][1]) + sh.d[par][k][2]) + sh.d[par][k][3];
  par ^= 1;
}
__device__ __forceinline__ float block_max(float v, SampleShared& sh, int& par) {
  v = warp_max(v);
  if ((threadIdx.x & 63) == 0) sh.f[par][threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(sh.f[par][0], sh.f[par][1]), fmaxf(sh.f[par][2], sh.f[par][3]));
  par ^= 1;
  return r;
}
// three counts of at most 2^20 each, packed into 21-bit fields of one 64-bit word
__device__ __forceinline__ unsigned long long block_count3(unsigned long long v, SampleShared& sh, int& par) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh.q[par][threadIdx.x >> 6] = v;
  __syncthreads();
  const unsigned long long r = sh.q[par][0] + sh.q[par][1] + sh.q[par][2] + sh.q[par][3];
  par ^= 1;
  return r;
}

// weight of an element relative to the row maximum m: 1 at the maximum (also when m is +inf), exp(z - m) below
__device__ __forceinline__ float weight(float z, float m) { return z == m ? 1.0f : expf(z - m); }

// Steps 1, 3 and 7 of the rule, shared by the sampler and by the scoring kernel (mmt_score_multi), so a score is
// bit for bit the log-probability the sampler writes for the same row and token.
// step 1: z = logit * inv_t (one fp32 multiply), NaN as -inf
__device__ __forceinline__ float scaled_logit(const float* __restrict__ row, int i, float inv_t) {
  const float z = row[i] * inv_t;
  return z != z ? -INFINITY : z;
}
// step 1 over the row: the scaled logits into LDS (ONCHIP) and their maximum; the barrier of the reduction also
// publishes zs
template <bool ONCHIP>
__device__ __forceinline__ float row_max(float* __restrict__ zs, const float* __restrict__ row, int V, float inv_t,
                                         SampleShared& sh, int& par) {
  float m = -INFINITY;
  for (int i = threadIdx.x; i < V; i += SAMPLE_THREADS) {
    const float z = scaled_logit(row, i, inv_t);
    if (ONCHIP) zs[i] = z;
    m = fmaxf(m, z);
  }
  return block_max(m, sh, par);
}
// steps 3, 5: the weights of { key >= K } summed in vocabulary order. Thread t owns the contiguous chunk
// [t c, t c + c), c odd so the LDS reads of a wave spread over the banks; serial sum per thread, shift scan over
// the lanes, wave totals added left to right. Every thread ends with S, its own total and its exclusive prefix.
struct RowSums {
  int i0, i1;
  double tot, base, S;
  bool has_max;
};
template <class ZAT>
__device__ __forceinline__ RowSums row_sums(ZAT zat, int V, float m, uint32_t K, SampleShared& sh, int& par) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  RowSums r;
  const int c = ((V + SAMPLE_THREADS - 1) / SAMPLE_THREADS) | 1;
  const int64_t i0l = (int64_t)tid * c;
  r.i0 = i0l < V ? (int)i0l : V;
  r.i1 = i0l + c < V ? (int)(i0l + c) : V;
  r.tot = 0.0;
  r.has_max = false;
  for (int i = r.i0; i < r.i1; ++i) {
    const float z = zat(i);
    r.tot += okey(z) >= K ? (double)weight(z, m) : 0.0;
    r.has_max = r.has_max || z == m;
  }
  double inc = r.tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  double ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = 0.0;
  if (lane == 63) sh.d[par][0][wave] = inc;
  __syncthreads();
  const double w0 = sh.d[par][0][0], w1 = sh.d[par][0][1], w2 = sh.d[par][0][2], w3 = sh.d[par][0][3];
  par ^= 1;
  r.S = ((w0 + w1) + w2) + w3;
  const double wbase = wave == 0 ? 0.0 : wave == 1 ? w0 : wave == 2 ? (w0 + w1) : ((w0 + w1) + w2);
  r.base = wbase + ex;
  return r;
}
// step 7: log(e_tok / S) = (z_tok - m) - log S, rounded to fp32 once
__device__ __forceinline__ float token_logprob(float zt, float m, double S) {
  const float d = zt == m ? 0.f : zt - m;
  return (float)((double)d - log(S));
}

// Steps 1 - 4 and the sums of step 5 for one row: the law the row's token is drawn from. The scaled logits (in LDS
// when ONCHIP), their maximum m, the threshold key K of top-k then top-p (0 keeps everything; greedy leaves it 0)
// and row_sums over { key >= K }: e_i = weight(z_i, m) there and 0 elsewhere, P(i) = e_i / S. A row with no finite
// logit has m == -inf and no law: the function returns right after the maximum, K and rs unset (a uniform branch:
// every thread holds m). The sampler goes on to the draw from here, the forecast kernel keeps (m, K, S).
struct RowLaw {
  float m;
  uint32_t K;
  RowSums rs;
};
template <bool ONCHIP, class ZAT>
__device__ __forceinline__ RowLaw row_law(ZAT zat, float* __restrict__ zs, const float* __restrict__ row, int V,
                                          float inv_t, int greedy, int top_k, float top_p, SampleShared& sh,
                                          int& par) {
  const int tid = threadIdx.x;
  RowLaw law;
  const float m = row_max<ONCHIP>(zs, row, V, inv_t, sh, par);
  law.m = m;
  law.K = 0;
  if (m == -INFINITY) return law;

  // step 2: top-k threshold key, the k-th largest key (duplicates counted); 0 keeps everything
  uint32_t K = 0;
  if (!greedy && top_k > 0 && top_k < V) {
    for (int bit = 30; bit >= 0; bit -= 2) {  // two bits per round: the largest of three candidates that holds
      const uint32_t c1 = K | (1u << bit), c2 = K | (2u << bit), c3 = K | (3u << bit);
      unsigned long long n = 0;
      for (int i = tid; i < V; i += SAMPLE_THREADS) {
        const uint32_t k = okey(zat(i));
        n += (k >= c1 ? 1ull : 0ull) + (k >= c2 ? 1ull << 21 : 0ull) + (k >= c3 ? 1ull << 42 : 0ull);
      }
      n = block_count3(n, sh, par);
      const unsigned long long kk = (unsigned long long)top_k;
      K = (n >> 42) >= kk ? c3 : ((n >> 21) & 0x1FFFFFull) >= kk ? c2 : (n & 0x1FFFFFull) >= kk ? c1 : K;
    }
  }

  // steps 3, 4: the mass of { key >= max(cand, K) } over the interleaved assignment; top-p threshold key
  if (!greedy && top_p < 1.0f) {
    const uint32_t km = okey(m);
    if (top_p <= 0.0f) {
      K = km;
    } else {
      // s[j] = mass of { key >= l_j } for l1 <= l2 <= l3: each a sum over the same assignment and tree with the
      // leaves below its bound zeroed
      auto mass3 = [&](uint32_t l1, uint32_t l2, uint32_t l3, double (&s)[3]) {
        s[0] = s[1] = s[2] = 0.0;
        for (int i = tid; i < V; i += SAMPLE_THREADS) {
          const float z = zat(i);
          const uint32_t k = okey(z);
          if (k >= l1) {
            const double w = (double)weight(z, m);
            s[0] += w;
            s[1] += k >= l2 ? w : 0.0;
            s[2] += k >= l3 ? w : 0.0;
          }
        }
        block_sum3(s, sh, par);
      };
      double s[3];
      mass3(K, 0xFFFFFFFFu, 0xFFFFFFFFu, s);  // no key is 0xFFFFFFFF (a NaN pattern; NaNs were replaced)
      const double pS = (double)top_p * s[0];
      uint32_t P = 0;
      for (int bit = 30; bit >= 0; bit -= 2) {
        const uint32_t c1 = P | (1u << bit), c2 = P | (2u << bit), c3 = P | (3u << bit);
        mass3(c1 > K ? c1 : K, c2 > K ? c2 : K, c3 > K ? c3 : K, s);
        P = s[2] >= pS ? c3 : s[1] >= pS ? c2 : s[0] >= pS ? c1 : P;
      }
      K = P > K ? P : K;
      K = K < km ? K : km;  // the maximal group always stays
    }
  }

  // steps 5, 6: prefix sums in vocabulary order (row_sums)
  law.K = K;
  law.rs = row_sums(zat, V, m, K, sh, par);
  return law;
}

}  // namespace
