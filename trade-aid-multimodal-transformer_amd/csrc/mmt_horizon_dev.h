// Device code shared by mmt_horizon.hip (mmt_horizon_stats) and mmt_horizon_score.hip (mmt_horizon_score): the rule-1
// walk of one token row, the weight rule, the chunk tree, the bitonic sort of (x, s) and the prefix of the weights in
// sorted order. Both files give the bits the rules in mmt.h state, so whatever one of them computes with these
// functions compares exactly against the other's.
//
// Rule 1 is one IEEE operation per line: floating-point contraction is off from here to the end of the including
// file, or the compiler fuses g * u - 1 into one multiply-add and x loses its bits against the rule (and against any
// other implementation).
#pragma once
#include <cmath>

#include "mmt_common.h"
#include "mmt_kernels.h"
#include "mmt_sample_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int HZ_MAX_S = 4096;  // the rows of a (prompt, step) are sorted in LDS (mmt_resample's cap)
constexpr int HZ_THREADS = SAMPLE_THREADS;
constexpr int HZ_WAVES = SAMPLE_WAVES;
constexpr int HZ_NSUM = 11 + MMT_HZ_MAX_B;

// the scratch of problem `index`: x, hi, lo fp64 [steps][rows], d int8 [steps][rows], dead int32 [rows]
struct HzScratch {
  char* base;
  int64_t rows, cells, per;  // cells = steps * rows; per = bytes of one problem
  __host__ __device__ double* x(int index) const { return reinterpret_cast<double*>(base + index * per); }
  __host__ __device__ double* hi(int index) const { return x(index) + cells; }
  __host__ __device__ double* lo(int index) const { return x(index) + 2 * cells; }
  __host__ __device__ int8_t* d(int index) const { return reinterpret_cast<int8_t*>(x(index) + 3 * cells); }
  __host__ __device__ int32_t* dead(int index) const {
    return reinterpret_cast<int32_t*>(base + index * per + 24 * cells + ((cells + 15) & ~(int64_t)15));
  }
  // the bytes of the five arrays above, a multiple of 16
  __host__ __device__ int64_t walk_bytes() const {
    return 24 * cells + ((cells + 15) & ~(int64_t)15) + ((4 * rows + 15) & ~(int64_t)15);
  }
};

__device__ __forceinline__ int hz_sign(double v) { return v > 0.0 ? 1 : v < 0.0 ? -1 : 0; }

// Rule 1 for one row: tk its `steps` tokens, org its origin token (not read for a percent series). Leaves x, hi, lo
// and d of step j at [j * stride] and returns false for a dead row, which stops at its first bad token.
__device__ __forceinline__ bool hz_walk_row(const int64_t* __restrict__ tk, const int64_t* org,
                                            const double* __restrict__ val, int V, int pct, int steps, double* xs,
                                            double* his, double* los, int8_t* ds, int64_t stride) {
  bool ok = true;
  double v0 = 0.0;
  if (!pct) {
    const int64_t o = *org;
    ok = o >= 0 && o < V;
    if (ok) v0 = val[o];
  }
  double prev = v0, g = 1.0, h = 0.0, l = 0.0;
  for (int j = 0; ok && j < steps; ++j) {
    const int64_t t = tk[j];
    if (t < 0 || t >= V) { ok = false; break; }
    const double v = val[t];
    double x;
    int d;
    if (pct) {
      const double c = v / 100.0;
      const double u = 1.0 + c;
      g = g * u;  // g_0 = 1 * u = u exactly
      const double e = g - 1.0;
      x = e * 100.0;
      d = hz_sign(v);
    } else {
      x = v - v0;
      d = hz_sign(v - prev);
      prev = v;
    }
    if (!(fabs(x) < INFINITY)) { ok = false; break; }
    h = fmax(h, x);
    l = fmin(l, x);
    const int64_t at = (int64_t)j * stride;
    xs[at] = x;
    his[at] = h;
    los[at] = l;
    ds[at] = (int8_t)d;
  }
  return ok;
}

struct HzShared {
  double d[2][HZ_NSUM][HZ_WAVES];
  int i[2][MMT_HZ_MAX_Q][HZ_WAVES];
};

// the chunk tree for N sums at once: a thread's serial totals in, the block totals out (one barrier)
template <int N>
__device__ __forceinline__ void hz_sums(double (&v)[N], int n, HzShared& sh, int& par) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {  // unrolled: v stays in registers
    if (k >= n) continue;
    double inc = v[k];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double m = __shfl_up(inc, o, 64);
      if (lane >= o) inc += m;
    }
    if (lane == 63) sh.d[par][k][wave] = inc;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k)
    if (k < n) v[k] = ((sh.d[par][k][0] + sh.d[par][k][1]) + sh.d[par][k][2]) + sh.d[par][k][3];
  par ^= 1;
}

// an int summed over the block (one barrier)
__device__ __forceinline__ int hz_count(int n, HzShared& sh, int& par) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if (lane == 0) sh.i[par][0][wave] = n;
  __syncthreads();
  n = sh.i[par][0][0] + sh.i[par][0][1] + sh.i[par][0][2] + sh.i[par][0][3];
  par ^= 1;
  return n;
}

// the log-weight of local row s as rule 2 reads it: NaN and dead rows count as -inf
__device__ __forceinline__ double hz_logw(const double* __restrict__ logw, const int32_t* __restrict__ dead, int64_t r0,
                                          int s) {
  double a = logw ? logw[r0 + s] : 0.0;
  if (a != a || dead[s]) a = -INFINITY;
  return a;
}

// rule 2, first half: the largest log-weight over the rows that are not dead (-inf: no live path; one barrier)
__device__ __forceinline__ double hz_weight_max(const double* __restrict__ logw, const int32_t* __restrict__ dead,
                                                int64_t r0, int S, HzShared& sh, int& par) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double mx = -INFINITY;
  for (int s = tid; s < S; s += HZ_THREADS) mx = fmax(mx, hz_logw(logw, dead, r0, s));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) sh.d[par][0][wave] = mx;
  __syncthreads();
  mx = fmax(fmax(sh.d[par][0][0], sh.d[par][0][1]), fmax(sh.d[par][0][2], sh.d[par][0][3]));
  par ^= 1;
  return mx;
}

// rule 2, second half: the fp32 weights of the prompt's rows into LDS (one barrier)
__device__ __forceinline__ void hz_weight_fill(const double* __restrict__ logw, const int32_t* __restrict__ dead,
                                               int64_t r0, int S, double mx, float* es) {
  for (int s = threadIdx.x; s < S; s += HZ_THREADS) {
    const double a = hz_logw(logw, dead, r0, s);
    float e = 0.f;
    if (a != -INFINITY) {
      const float d = (float)(a - mx);
      e = d == 0.f ? 1.0f : expf(d);
    }
    es[s] = e;
  }
  __syncthreads();
}

// rule 4's order: (x, s) ascending in LDS; rows without weight and the padding to a power of two sort last (+inf, and
// an index no smaller than any row's)
__device__ __forceinline__ void hz_sort(const double* __restrict__ xs, const float* es, int S, double* key,
                                        uint16_t* ix) {
  const int tid = threadIdx.x;
  int n2 = 1;
  while (n2 < S) n2 <<= 1;
  for (int i = tid; i < n2; i += HZ_THREADS) {
    key[i] = (i < S && es[i] > 0.f) ? xs[i] : INFINITY;
    ix[i] = (uint16_t)i;
  }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += HZ_THREADS) {
        const int lo_i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), hi_i = lo_i | jj;
        const double ka = key[lo_i], kb = key[hi_i];
        const uint16_t ia = ix[lo_i], ib = ix[hi_i];
        const bool gt = ka > kb || (ka == kb && ia > ib);
        if (gt == ((lo_i & k) == 0)) {
          key[lo_i] = kb; key[hi_i] = ka;
          ix[lo_i] = ib; ix[hi_i] = ia;
        }
      }
      __syncthreads();
    }
}

// the exclusive prefix, before place p0, of the weights in sorted order over the chunk tree: thread t owns the places
// p0..p1-1 (one barrier). The inclusive prefix through place i is this plus the thread's serial sum through i.
__device__ __forceinline__ double hz_sorted_prefix(const float* es, const uint16_t* ix, int p0, int p1, HzShared& sh,
                                                   int& par) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double inc = 0.0;
  for (int i = p0; i < p1; ++i) inc += (double)es[ix[i]];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double m = __shfl_up(inc, o, 64);
    if (lane >= o) inc += m;
  }
  double ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = 0.0;
  if (lane == 63) sh.d[par][0][wave] = inc;
  __syncthreads();
  {
    const double w0 = sh.d[par][0][0], w1 = sh.d[par][0][1], w2 = sh.d[par][0][2];
    ex += wave == 0 ? 0.0 : wave == 1 ? w0 : wave == 2 ? (w0 + w1) : ((w0 + w1) + w2);
  }
  par ^= 1;
  return ex;
}

}  // namespace
