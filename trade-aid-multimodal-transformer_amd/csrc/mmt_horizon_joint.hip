// Joint horizon forecasts of rollouts (mmt.h: mmt_horizon_joint): what mmt_horizon_stats says of one series, said of
// several at once over the same paths: where a basket sum_p coef_p x^(p) stands after j steps (moments, sign masses,
// quantiles, the tail mean below each quantile, barrier hits), and per pair of series the covariance, the correlation
// and the 3 x 3 tables of their signs and step directions.
//
// Three launches (one chunk: at most 8 problems, 8 baskets, 28 pairs):
//   walk     grid ceil(rows / 256), 256 threads: thread r runs rule 1 (hz_walk_row) for every problem of its row, x
//            (fp64) and d (int8) of each into the scratch, step-major; hz_walk_row's hi / lo go to two spare planes
//            that are never read. A row that is alive in every problem then forms its baskets from the x it wrote: y,
//            hi^y, lo^y per (basket, step). One dead flag per row: dead in any problem, or a y that is not finite.
//   baskets  grid (prompts x steps, nbk), 256 threads: mmt_horizon.hip's reduce on y (weights, sums over the chunk
//            tree, bitonic sort of (y, s) in LDS, prefix of the weights in sorted order) plus the prefix of w y over
//            the same tree for the tail means. LDS as there: 32 + 8 + 16 KiB at 4096 rows and the reduction slots.
//   pairs    grid (prompts x steps, npair), 256 threads: the weights in LDS (16 KiB), x_p, x_q, d_p, d_q streamed from
//            the scratch twice: W, Q, the two means and the sign table behind one barrier, the step table behind a
//            second, then the three central sums.
// No float atomics, no data-dependent order of a sum: bit-identical run to run; a (prompt, step, basket | pair) reads
// its own rows only. The weights, W, Q and the per-series sums are formed as mmt_horizon.hip forms them, so with no
// dead row ess, live, a pair's variances and a unit basket's sums carry mmt_horizon_stats' bits.
//
// Every line of the rule is one IEEE operation: floating-point contraction is off for this file, or the compiler fuses
// y + coef * x into one multiply-add and y loses its bits against the rule.
#include <cmath>

#include "mmt.h"
#include "mmt_common.h"
#include "mmt_kernels.h"
#include "mmt_horizon_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int HJ_MAX_P = 8, HJ_MAX_K = 8, HJ_MAX_PAIR = 28;

// the scratch: x fp64 [count][steps][rows], y / hi / lo fp64 [nbk][3][steps][rows], two spare fp64 planes, d int8
// [count][steps][rows] (each plane padded to 16 bytes), dead int32 [rows]
struct HjScratch {
  char* base;
  int64_t rows, cells;  // cells = steps * rows
  int32_t count, nbk;
  __host__ __device__ int64_t dpad() const { return (cells + 15) & ~(int64_t)15; }
  __host__ __device__ double* x(int p) const { return reinterpret_cast<double*>(base) + p * cells; }
  __host__ __device__ double* y(int k) const { return x(count) + 3 * k * cells; }
  __host__ __device__ double* hi(int k) const { return y(k) + cells; }
  __host__ __device__ double* lo(int k) const { return y(k) + 2 * cells; }
  __host__ __device__ double* spare(int i) const { return x(count) + (3 * nbk + i) * cells; }
  __host__ __device__ int8_t* d(int p) const { return reinterpret_cast<int8_t*>(spare(2)) + p * dpad(); }
  __host__ __device__ int32_t* dead() const { return reinterpret_cast<int32_t*>(d(count)); }
  __host__ __device__ int64_t bytes() const {
    return 8 * cells * (count + 3 * nbk + 2) + count * dpad() + ((4 * rows + 15) & ~(int64_t)15);
  }
};

struct HjProblem {
  const int64_t* tok; int64_t tok_stride;
  const double* values;
  const int64_t* origin; int64_t origin_stride;  // not read for a percent series
  int V, is_percent;
};
struct HjWalk { HjProblem p[HJ_MAX_P]; double coef[HJ_MAX_K][HJ_MAX_P]; };
struct HjBaskets {
  double* bstats[HJ_MAX_K]; double* bqval[HJ_MAX_K]; int32_t* bqrow[HJ_MAX_K]; double* btail[HJ_MAX_K];
  double* bhit[HJ_MAX_K];
  double barrier[HJ_MAX_K][MMT_HZ_MAX_B];
  double level[MMT_HZ_MAX_Q];
  double* ess; int32_t* live;  // nullable
  int nq, nb;
};
struct HjPairs {
  double* pstats[HJ_MAX_PAIR];
  int32_t pair[HJ_MAX_PAIR][2];
  double* ess; int32_t* live;  // nullable; null too when the basket launch writes them
};

bool hj_plan(int32_t count, int32_t batch, int32_t samples, int32_t steps, int32_t nbk, HjScratch& sc) {
  if (count < 0 || batch < 0 || steps < 0 || samples < 1 || (int64_t)batch * samples > 0x7fffffff) return false;
  if (count > HJ_MAX_P || nbk < 0 || nbk > HJ_MAX_K) return false;
  sc.base = nullptr;
  sc.rows = (int64_t)batch * samples;
  sc.cells = sc.rows * steps;
  sc.count = count;
  sc.nbk = nbk;
  return sc.cells <= ((int64_t)1 << 44);  // under 300 bytes a cell: far past any device, and no overflow in bytes()
}

__global__ __launch_bounds__(HZ_THREADS) void joint_walk_kernel(HjWalk a, HjScratch sc, int steps) {
  const int64_t r = (int64_t)blockIdx.x * HZ_THREADS + threadIdx.x;
  if (r >= sc.rows) return;
  bool ok = true;
  for (int p = 0; ok && p < sc.count; ++p) {
    const HjProblem& q = a.p[p];
    ok = hz_walk_row(q.tok + r * q.tok_stride, q.is_percent ? nullptr : q.origin + r * q.origin_stride, q.values, q.V,
                     q.is_percent, steps, sc.x(p) + r, sc.spare(0) + r, sc.spare(1) + r, sc.d(p) + r, sc.rows);
  }
  // the baskets of a row every series of which is alive, from the x this thread has just written
  for (int k = 0; ok && k < sc.nbk; ++k) {
    double* ys = sc.y(k) + r;
    double* his = sc.hi(k) + r;
    double* los = sc.lo(k) + r;
    double h = 0.0, l = 0.0;
    for (int j = 0; j < steps; ++j) {
      const int64_t at = (int64_t)j * sc.rows;
      double y = 0.0;
      for (int p = 0; p < sc.count; ++p) {
        const double t = a.coef[k][p] * sc.x(p)[at + r];
        y = y + t;
      }
      if (!(fabs(y) < INFINITY)) { ok = false; break; }
      h = fmax(h, y);
      l = fmin(l, y);
      ys[at] = y;
      his[at] = h;
      los[at] = l;
    }
  }
  sc.dead()[r] = ok ? 0 : 1;
}

// the exclusive prefixes, before place p0, of w and of w y in sorted order over hz_sorted_prefix's tree, behind one
// barrier: returns that of w (hz_sorted_prefix's bits) and leaves that of w y (one product per row) in exa
__device__ __forceinline__ double hj_sorted_prefix(const float* es, const uint16_t* ix, const double* key, int p0,
                                                   int p1, HzShared& sh, int& par, double& exa) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double inc = 0.0, ina = 0.0;
  for (int i = p0; i < p1; ++i) {
    const double w = (double)es[ix[i]];
    const double t = w * key[i];
    inc += w;
    ina += t;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double m = __shfl_up(inc, o, 64), n = __shfl_up(ina, o, 64);
    if (lane >= o) { inc += m; ina += n; }
  }
  double ex = __shfl_up(inc, 1, 64), ea = __shfl_up(ina, 1, 64);
  if (lane == 0) { ex = 0.0; ea = 0.0; }
  if (lane == 63) { sh.d[par][0][wave] = inc; sh.d[par][1][wave] = ina; }
  __syncthreads();
  {
    const double w0 = sh.d[par][0][0], w1 = sh.d[par][0][1], w2 = sh.d[par][0][2];
    ex += wave == 0 ? 0.0 : wave == 1 ? w0 : wave == 2 ? (w0 + w1) : ((w0 + w1) + w2);
    const double a0 = sh.d[par][1][0], a1 = sh.d[par][1][1], a2 = sh.d[par][1][2];
    ea += wave == 0 ? 0.0 : wave == 1 ? a0 : wave == 2 ? (a0 + a1) : ((a0 + a1) + a2);
  }
  par ^= 1;
  exa = ea;
  return ex;
}

__global__ __launch_bounds__(HZ_THREADS) void joint_basket_kernel(HjBaskets a, HjScratch sc, int S, int steps,
                                                                  const double* __restrict__ logw) {
  __shared__ double key[HZ_MAX_S];
  __shared__ float es[HZ_MAX_S];
  __shared__ uint16_t ix[HZ_MAX_S];
  __shared__ HzShared sh;
  const int kb = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nq = a.nq, nb = a.nb;
  const int b = blockIdx.x / steps, j = blockIdx.x % steps;
  const int64_t r0 = (int64_t)b * S, cell = (int64_t)j * sc.rows + r0, out = (int64_t)b * steps + j;
  const double* __restrict__ ys = sc.y(kb) + cell;
  const double* __restrict__ his = sc.hi(kb) + cell;
  const double* __restrict__ los = sc.lo(kb) + cell;
  const int32_t* __restrict__ dead = sc.dead() + r0;
  double* st = a.bstats[kb] + out * 9;
  const bool first = j == 0 && kb == 0 && tid == 0;  // the workgroup that writes the prompt's ess and live
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  int par = 0;

  // rule 2 over the rows that are dead in no series
  const double mx = hz_weight_max(logw, dead, r0, S, sh, par);
  if (mx == -INFINITY) {  // no live path (uniform branch)
    if (tid < 9) st[tid] = nan;
    if (tid < nq) {
      a.bqval[kb][out * nq + tid] = nan;
      a.bqrow[kb][out * nq + tid] = -1;
      a.btail[kb][out * nq + tid] = nan;
    }
    if (tid < nb) a.bhit[kb][out * nb + tid] = nan;
    if (first) {
      if (a.ess) a.ess[b] = 0.0;
      if (a.live) a.live[b] = 0;
    }
    return;
  }
  hz_weight_fill(logw, dead, r0, S, mx, es);

  // rules 3 and 6: the sums in row order over the chunk tree
  const int c = ((S + HZ_THREADS - 1) / HZ_THREADS) | 1;
  const int i0 = min(tid * c, S), i1 = min(tid * c + c, S);
  double v[8 + MMT_HZ_MAX_B];
#pragma unroll
  for (int k = 0; k < 8 + MMT_HZ_MAX_B; ++k) v[k] = 0.0;
  int live = 0;
  for (int i = i0; i < i1; ++i) {
    const float e = es[i];
    if (!(e > 0.f)) continue;  // a dead row's cells were never written
    const double w = (double)e, y = ys[i], h = his[i], l = los[i];
    ++live;
    v[0] += w;
    v[1] += w * w;  // the product of two fp32 values is exact in fp64
    v[2] += w * y;
    v[3] += y < 0.0 ? w : 0.0;
    v[4] += y == 0.0 ? w : 0.0;
    v[5] += y > 0.0 ? w : 0.0;
    v[6] += w * h;
    v[7] += w * l;
#pragma unroll
    for (int k = 0; k < MMT_HZ_MAX_B; ++k) {
      const double u = a.barrier[kb][k];
      if (k < nb) v[8 + k] += (u > 0.0 ? h >= u : l <= u) ? w : 0.0;
    }
  }
  hz_sums(v, 8 + nb, sh, par);
  live = hz_count(live, sh, par);
  const double W = v[0], mean = v[2] / W;
  double var[1] = {0.0};
  for (int i = i0; i < i1; ++i) {
    const float e = es[i];
    if (!(e > 0.f)) continue;
    const double dv = ys[i] - mean;
    var[0] += (double)e * (dv * dv);
  }
  hz_sums(var, 1, sh, par);

  // rule 4: (y, s) ascending; rows without weight and the padding sort last
  hz_sort(ys, es, S, key, ix);
  if (tid == 0) {
    st[0] = mean;
    st[1] = var[0] / W;
    st[2] = v[3] / W;
    st[3] = v[4] / W;
    st[4] = v[5] / W;
    st[5] = v[6] / W;
    st[6] = v[7] / W;
    st[7] = key[0];
    st[8] = key[live - 1];
    if (first) {
      if (a.ess) a.ess[b] = W * W / v[1];
      if (a.live) a.live[b] = live;
    }
  }
#pragma unroll
  for (int k = 0; k < MMT_HZ_MAX_B; ++k)
    if (tid == k && k < nb) a.bhit[kb][out * nb + k] = v[8 + k] / W;
  if (nq == 0) return;

  // the prefixes of w and w y in sorted order over the same tree, on the first `live` places
  const int p0 = min(tid * c, live), p1 = min(tid * c + c, live);
  double exa;
  const double ex = hj_sorted_prefix(es, ix, key, p0, p1, sh, par, exa);
  for (int k = 0; k < nq; ++k) {
    const double target = a.level[k] * W;
    int pos = live;
    double p = ex;
    for (int i = p0; i < p1; ++i) {
      p += (double)es[ix[i]];
      if (p >= target) { pos = i; break; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pos = min(pos, __shfl_xor(pos, o, 64));
    if (lane == 0) sh.i[par][k][wave] = pos;
  }
  __syncthreads();
  for (int k = 0; k < nq; ++k) {
    int pos = min(min(sh.i[par][k][0], sh.i[par][k][1]), min(sh.i[par][k][2], sh.i[par][k][3]));
    if (pos >= live) pos = live - 1;  // rounding left no such row: the last row with weight
    if (pos < p0 || pos >= p1) continue;  // the thread that owns the place writes it
    // rule 5: P and A through the place before the quantile row's
    double P = ex, A = exa;
    for (int i = p0; i < pos; ++i) {
      const double w = (double)es[ix[i]];
      const double t = w * key[i];
      P += w;
      A += t;
    }
    const double target = a.level[k] * W;
    const double rem = target - P;
    const double t = rem * key[pos];
    const double num = A + t;
    a.bqrow[kb][out * nq + k] = ix[pos];
    a.bqval[kb][out * nq + k] = key[pos];
    a.btail[kb][out * nq + k] = num / target;
  }
}

__global__ __launch_bounds__(HZ_THREADS) void joint_pair_kernel(HjPairs a, HjScratch sc, int S, int steps,
                                                                const double* __restrict__ logw) {
  __shared__ float es[HZ_MAX_S];
  __shared__ HzShared sh;
  const int pp = a.pair[blockIdx.y][0], pq = a.pair[blockIdx.y][1];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / steps, j = blockIdx.x % steps;
  const int64_t r0 = (int64_t)b * S, cell = (int64_t)j * sc.rows + r0, out = (int64_t)b * steps + j;
  const double* __restrict__ xp = sc.x(pp) + cell;
  const double* __restrict__ xq = sc.x(pq) + cell;
  const int8_t* __restrict__ dp = sc.d(pp) + cell;
  const int8_t* __restrict__ dq = sc.d(pq) + cell;
  const int32_t* __restrict__ dead = sc.dead() + r0;
  double* st = a.pstats[blockIdx.y] + out * 22;
  const bool first = j == 0 && blockIdx.y == 0 && tid == 0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  int par = 0;

  const double mx = hz_weight_max(logw, dead, r0, S, sh, par);
  if (mx == -INFINITY) {  // no live path (uniform branch)
    if (tid < 22) st[tid] = nan;
    if (first) {
      if (a.ess) a.ess[b] = 0.0;
      if (a.live) a.live[b] = 0;
    }
    return;
  }
  hz_weight_fill(logw, dead, r0, S, mx, es);

  // first pass: W, Q, the two means' sums and the sign table behind one barrier, the step table behind the next
  const int c = ((S + HZ_THREADS - 1) / HZ_THREADS) | 1;
  const int i0 = min(tid * c, S), i1 = min(tid * c + c, S);
  double v[13], t9[9];
#pragma unroll
  for (int k = 0; k < 13; ++k) v[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) t9[k] = 0.0;
  int live = 0;
  for (int i = i0; i < i1; ++i) {
    const float e = es[i];
    if (!(e > 0.f)) continue;  // a dead row's cells were never written
    const double w = (double)e, x = xp[i], z = xq[i];
    const int cs = 3 * (hz_sign(x) + 1) + (hz_sign(z) + 1), cd = 3 * (dp[i] + 1) + (dq[i] + 1);
    ++live;
    v[0] += w;
    v[1] += w * w;  // the product of two fp32 values is exact in fp64
    v[2] += w * x;
    v[3] += w * z;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      v[4 + k] += cs == k ? w : 0.0;
      t9[k] += cd == k ? w : 0.0;
    }
  }
  hz_sums(v, 13, sh, par);
  hz_sums(t9, 9, sh, par);
  live = hz_count(live, sh, par);
  const double W = v[0], mp = v[2] / W, mq = v[3] / W;

  // second pass: the central sums, the product of the two deviations first, then the weight (rule 3's variance)
  double u[3] = {0.0, 0.0, 0.0};
  for (int i = i0; i < i1; ++i) {
    const float e = es[i];
    if (!(e > 0.f)) continue;
    const double w = (double)e, da = xp[i] - mp, dc = xq[i] - mq;
    u[0] += w * (da * da);
    u[1] += w * (dc * dc);
    u[2] += w * (da * dc);
  }
  hz_sums(u, 3, sh, par);
  if (tid == 0) {
    const double cov = u[2] / W, vp = u[0] / W, vq = u[1] / W;
    const double den = sqrt(vp) * sqrt(vq);
    st[0] = cov;
    st[1] = den == 0.0 ? nan : cov / den;
    st[2] = vp;
    st[3] = vq;
    if (first) {
      if (a.ess) a.ess[b] = W * W / v[1];
      if (a.live) a.live[b] = live;
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k)
    if (tid == 1 + k) {
      st[4 + k] = v[4 + k] / W;
      st[13 + k] = t9[k] / W;
    }
}

}  // namespace

extern "C" {

int64_t mmt_horizon_joint_scratch_bytes(int32_t count, int32_t batch, int32_t samples, int32_t steps, int32_t nbk) {
  HjScratch sc;
  if (!hj_plan(count, batch, samples, steps, nbk, sc)) return -1;
  if (samples > HZ_MAX_S) return -1;
  return sc.bytes();
}

int mmt_horizon_joint(void* stream, int32_t count, int32_t batch, int32_t samples, int32_t steps, const int32_t* V,
                      const int64_t* const* tok, const int64_t* tok_stride, const double* const* values,
                      const int32_t* is_percent, const int64_t* const* origin, const int64_t* origin_stride,
                      const double* logw, int32_t nq, const double* levels, int32_t nbk, const double* coef, int32_t nb,
                      const double* barriers, int32_t npair, const int32_t* pairs, double* const* bstats,
                      double* const* bqval, int32_t* const* bqrow, double* const* btail, double* const* bhit,
                      double* const* pstats, double* ess, int32_t* live, void* scratch, int64_t scratch_bytes) {
  if (count < 0 || batch < 0 || steps < 0 || samples < 1) return MMT_ERR_INVALID;
  if ((int64_t)batch * samples > 0x7fffffff) return MMT_ERR_INVALID;
  if (nq < 0 || nq > MMT_HZ_MAX_Q || nb < 0 || nb > MMT_HZ_MAX_B) return MMT_ERR_INVALID;
  if (nbk < 0 || nbk > HJ_MAX_K || npair < 0 || npair > HJ_MAX_PAIR) return MMT_ERR_INVALID;
  if (nq > 0 && !levels) return MMT_ERR_INVALID;
  for (int k = 0; k < nq; ++k)
    if (!(levels[k] > 0.0 && levels[k] < 1.0)) return MMT_ERR_INVALID;
  if (nbk == 0 && npair == 0) return MMT_OK;
  if (nbk > 0) {
    if (!coef || !bstats || (nq > 0 && (!bqval || !bqrow || !btail)) || (nb > 0 && (!bhit || !barriers)))
      return MMT_ERR_INVALID;
    for (int k = 0; k < nbk; ++k) {
      bool any = false;
      for (int p = 0; p < count; ++p) {
        const double a = coef[(int64_t)k * count + p];
        if (!(std::fabs(a) < INFINITY)) return MMT_ERR_INVALID;
        any = any || a != 0.0;
      }
      if (!any) return MMT_ERR_INVALID;
      for (int i = 0; i < nb; ++i) {
        const double u = barriers[k * nb + i];
        if (!(std::fabs(u) < INFINITY) || u == 0.0) return MMT_ERR_INVALID;
      }
    }
  }
  if (npair > 0) {
    if (!pairs || !pstats) return MMT_ERR_INVALID;
    for (int k = 0; k < npair; ++k) {
      const int32_t p = pairs[2 * k], q = pairs[2 * k + 1];
      if (p < 0 || p >= count || q < 0 || q >= count || p == q) return MMT_ERR_INVALID;
    }
  }
  if (!V || !tok || !tok_stride || !values) return MMT_ERR_INVALID;
  const bool work = batch > 0 && steps > 0;
  for (int p = 0; p < count; ++p) {
    const bool pct = is_percent && is_percent[p];
    if (V[p] < 1 || tok_stride[p] < steps) return MMT_ERR_INVALID;
    if (!pct && (!origin || !origin_stride)) return MMT_ERR_INVALID;
    if (work && (!tok[p] || !values[p] || (!pct && !origin[p]))) return MMT_ERR_INVALID;
  }
  if (work) {
    for (int k = 0; k < nbk; ++k) {
      if (!bstats[k] || (nq > 0 && (!bqval[k] || !bqrow[k] || !btail[k])) || (nb > 0 && !bhit[k]))
        return MMT_ERR_INVALID;
    }
    for (int k = 0; k < npair; ++k)
      if (!pstats[k]) return MMT_ERR_INVALID;
  }
  if (count > HJ_MAX_P) return MMT_ERR_UNSUPPORTED;
  HjScratch sc;
  if (!hj_plan(count, batch, samples, steps, nbk, sc)) return MMT_ERR_INVALID;
  if (work && (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < sc.bytes())) return MMT_ERR_INVALID;
  for (int p = 0; p < count; ++p)
    if (V[p] > SAMPLE_MAX_V) return MMT_ERR_UNSUPPORTED;
  if (samples > HZ_MAX_S) return MMT_ERR_UNSUPPORTED;
  if ((int64_t)batch * steps > 0x7fffffff) return MMT_ERR_UNSUPPORTED;
  if (!work) return MMT_OK;

  sc.base = static_cast<char*>(scratch);
  hipStream_t s = (hipStream_t)stream;
  HjWalk wa;
  for (int k = 0; k < HJ_MAX_P; ++k) {
    const int p = k < count ? k : 0;
    HjProblem& q = wa.p[k];
    const bool pct = is_percent && is_percent[p];
    q.tok = tok[p];
    q.tok_stride = tok_stride[p];
    q.values = values[p];
    q.origin = pct ? nullptr : origin[p];
    q.origin_stride = pct ? 0 : origin_stride[p];
    q.V = V[p];
    q.is_percent = pct ? 1 : 0;
  }
  for (int k = 0; k < HJ_MAX_K; ++k)
    for (int p = 0; p < HJ_MAX_P; ++p) wa.coef[k][p] = (k < nbk && p < count) ? coef[(int64_t)k * count + p] : 0.0;
  hipLaunchKernelGGL(joint_walk_kernel, dim3((unsigned)((sc.rows + HZ_THREADS - 1) / HZ_THREADS)), dim3(HZ_THREADS), 0,
                     s, wa, sc, steps);
  if (hipGetLastError() != hipSuccess) return MMT_ERR_HIP;
  const unsigned cells = (unsigned)((int64_t)batch * steps);
  if (nbk > 0) {
    HjBaskets ba;
    for (int k = 0; k < HJ_MAX_K; ++k) {
      const int i = k < nbk ? k : 0;
      ba.bstats[k] = bstats[i];
      ba.bqval[k] = nq > 0 ? bqval[i] : nullptr;
      ba.bqrow[k] = nq > 0 ? bqrow[i] : nullptr;
      ba.btail[k] = nq > 0 ? btail[i] : nullptr;
      ba.bhit[k] = nb > 0 ? bhit[i] : nullptr;
      for (int u = 0; u < MMT_HZ_MAX_B; ++u) ba.barrier[k][u] = u < nb ? barriers[i * nb + u] : 1.0;
    }
    for (int k = 0; k < MMT_HZ_MAX_Q; ++k) ba.level[k] = k < nq ? levels[k] : 0.5;
    ba.ess = ess;
    ba.live = live;
    ba.nq = nq;
    ba.nb = nb;
    hipLaunchKernelGGL(joint_basket_kernel, dim3(cells, (unsigned)nbk), dim3(HZ_THREADS), 0, s, ba, sc, samples, steps,
                       logw);
    if (hipGetLastError() != hipSuccess) return MMT_ERR_HIP;
  }
  if (npair > 0) {
    HjPairs pa;
    for (int k = 0; k < HJ_MAX_PAIR; ++k) {
      const int i = k < npair ? k : 0;
      pa.pstats[k] = pstats[i];
      pa.pair[k][0] = pairs[2 * i];
      pa.pair[k][1] = pairs[2 * i + 1];
    }
    pa.ess = nbk > 0 ? nullptr : ess;  // the basket launch has written them
    pa.live = nbk > 0 ? nullptr : live;
    hipLaunchKernelGGL(joint_pair_kernel, dim3(cells, (unsigned)npair), dim3(HZ_THREADS), 0, s, pa, sc, samples, steps,
                       logw);
    if (hipGetLastError() != hipSuccess) return MMT_ERR_HIP;
  }
  return MMT_OK;
}

}  // extern "C"
