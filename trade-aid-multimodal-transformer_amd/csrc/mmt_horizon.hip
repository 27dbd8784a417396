// Horizon forecasts of rollouts (mmt.h: mmt_horizon_stats): where a series stands after j new steps on each path (the
// cumulative change against the path's origin, its running extremes, its step direction), and per (prompt, step) the
// weighted summaries of that quantity over the prompt's paths: moments, direction masses, quantiles, barrier hits.
//
// Two launches per chunk of 8 problems:
//   walk    grid (ceil(rows / 256), problems), 256 threads: thread (row, problem) runs rule 1 serially over the steps
//           and leaves x, hi, lo (fp64) and d (int8) in the scratch, step-major ([steps][rows]: the second stage reads
//           the rows of one (prompt, step) contiguously), plus the row's dead flag. A dead row stops at its first
//           bad token; what it left is never read.
//   reduce  grid (prompts x steps, problems), 256 threads: mmt_resample's rules 1 - 2 over the rows that are not dead
//           (the fp32 weights of the prompt in LDS), the sums of rules 3 and 5 over the resampler's chunk tree (thread t
//           owns the c = ceil(S / 256) | 1 rows from t c; serial sum, shift scan over the lanes, the four wave totals
//           left to right), then a bitonic sort of (x, s) in LDS, padded to a power of two with keys that sort last
//           (+inf, index >= the row's: rows without weight take that key too), and the prefix sums of the weights
//           in sorted order over the same tree for the quantiles.
// LDS of reduce at the cap of 4096 rows: fp64 keys 32 KiB + 16-bit indices 8 KiB + fp32 weights 16 KiB = 56 KiB, and
// under 2 KiB of reduction slots: inside the 64 KiB of a static allocation, two workgroups per CU.
// No float atomics, no data-dependent order of a sum: bit-identical run to run; a (prompt, step, problem) reads its own
// rows only.
//
// The device functions of every stage are in mmt_horizon_dev.h, which mmt_horizon_score.hip shares. Rule 1 is one IEEE
// operation per line: floating-point contraction is off for this file (the header turns it off for its own code), or
// the compiler fuses g * u - 1 into one multiply-add and x loses its bits against the rule.
#include <cmath>

#include "mmt.h"
#include "mmt_common.h"
#include "mmt_kernels.h"
#include "mmt_horizon_dev.h"

#pragma clang fp contract(off)

namespace {

bool hz_plan(int32_t count, int32_t batch, int32_t samples, int32_t steps, HzScratch& sc, int64_t& bytes) {
  if (count < 0 || batch < 0 || steps < 0 || samples < 1 || (int64_t)batch * samples > 0x7fffffff) return false;
  sc.rows = (int64_t)batch * samples;
  sc.cells = sc.rows * steps;
  if (sc.cells > ((int64_t)1 << 44)) return false;  // 25 bytes a cell: far past any device, and no overflow below
  sc.per = sc.walk_bytes();
  if (count > 0 && sc.per > (int64_t)0x7fffffffffffll / count) return false;
  bytes = sc.per * count;
  return true;
}

__global__ __launch_bounds__(HZ_THREADS) void horizon_walk_kernel(HorizonBatch batch, HzScratch sc, int steps) {
  const HorizonProblem& q = batch.p[blockIdx.y];
  const int64_t r = (int64_t)blockIdx.x * HZ_THREADS + threadIdx.x;
  if (r >= sc.rows) return;
  const bool ok = hz_walk_row(q.tok + r * q.tok_stride, q.is_percent ? nullptr : q.origin + r * q.origin_stride, q.values,
                              q.V, q.is_percent, steps, sc.x(q.index) + r, sc.hi(q.index) + r, sc.lo(q.index) + r,
                              sc.d(q.index) + r, sc.rows);
  sc.dead(q.index)[r] = ok ? 0 : 1;
}

__global__ __launch_bounds__(HZ_THREADS) void horizon_reduce_kernel(HorizonBatch batch, HzScratch sc, int S, int steps,
                                                                    const double* __restrict__ logw) {
  __shared__ double key[HZ_MAX_S];
  __shared__ float es[HZ_MAX_S];
  __shared__ uint16_t ix[HZ_MAX_S];
  __shared__ HzShared sh;
  const HorizonProblem& q = batch.p[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nq = batch.nq, nb = batch.nb;
  const int b = blockIdx.x / steps, j = blockIdx.x % steps;
  const int64_t r0 = (int64_t)b * S, cell = (int64_t)j * sc.rows + r0, out = (int64_t)b * steps + j;
  const double* __restrict__ xs = sc.x(q.index) + cell;
  const double* __restrict__ his = sc.hi(q.index) + cell;
  const double* __restrict__ los = sc.lo(q.index) + cell;
  const int8_t* __restrict__ ds = sc.d(q.index) + cell;
  const int32_t* __restrict__ dead = sc.dead(q.index) + r0;
  double* st = q.stats + out * 12;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  int par = 0;

  // rule 2: mmt_resample's rules 1 - 2 over the rows that are not dead
  const double mx = hz_weight_max(logw, dead, r0, S, sh, par);
  if (mx == -INFINITY) {  // no live path (uniform branch)
    if (tid < 12) st[tid] = nan;
    if (tid < nq) { q.qval[out * nq + tid] = nan; q.qrow[out * nq + tid] = -1; }
    if (tid < nb) q.hit[out * nb + tid] = nan;
    if (j == 0 && tid == 0) {
      if (q.ess) q.ess[b] = 0.0;
      if (q.live) q.live[b] = 0;
    }
    return;
  }
  hz_weight_fill(logw, dead, r0, S, mx, es);

  // rules 3 and 5: the sums in row order over the chunk tree
  const int c = ((S + HZ_THREADS - 1) / HZ_THREADS) | 1;
  const int i0 = min(tid * c, S), i1 = min(tid * c + c, S);
  double v[HZ_NSUM];
#pragma unroll
  for (int k = 0; k < HZ_NSUM; ++k) v[k] = 0.0;
  int live = 0;
  for (int i = i0; i < i1; ++i) {
    const float e = es[i];
    if (!(e > 0.f)) continue;  // a dead row's cells were never written
    const double w = (double)e, x = xs[i], h = his[i], l = los[i];
    const int d = ds[i];
    ++live;
    v[0] += w;
    v[1] += w * w;  // the product of two fp32 values is exact in fp64
    v[2] += w * x;
    v[3] += x < 0.0 ? w : 0.0;
    v[4] += x == 0.0 ? w : 0.0;
    v[5] += x > 0.0 ? w : 0.0;
    v[6] += d < 0 ? w : 0.0;
    v[7] += d == 0 ? w : 0.0;
    v[8] += d > 0 ? w : 0.0;
    v[9] += w * h;
    v[10] += w * l;
#pragma unroll
    for (int k = 0; k < MMT_HZ_MAX_B; ++k) {
      const double u = q.barrier[k];
      if (k < nb) v[11 + k] += (u > 0.0 ? h >= u : l <= u) ? w : 0.0;
    }
  }
  hz_sums(v, 11 + nb, sh, par);
  live = hz_count(live, sh, par);
  const double W = v[0], mean = v[2] / W;
  double var[1] = {0.0};
  for (int i = i0; i < i1; ++i) {
    const float e = es[i];
    if (!(e > 0.f)) continue;
    const double dv = xs[i] - mean;
    var[0] += (double)e * (dv * dv);
  }
  hz_sums(var, 1, sh, par);

  // rule 4: (x, s) ascending; rows without weight and the padding sort last
  hz_sort(xs, es, S, key, ix);
  if (tid == 0) {
    st[0] = mean;
    st[1] = var[0] / W;
#pragma unroll
    for (int k = 3; k <= 8; ++k) st[k - 1] = v[k] / W;
    st[8] = v[9] / W;
    st[9] = v[10] / W;
    st[10] = key[0];
    st[11] = key[live - 1];
    if (j == 0) {
      if (q.ess) q.ess[b] = W * W / v[1];
      if (q.live) q.live[b] = live;
    }
  }
#pragma unroll
  for (int k = 0; k < MMT_HZ_MAX_B; ++k)
    if (tid == k && k < nb) q.hit[out * nb + k] = v[11 + k] / W;
  if (nq == 0) return;

  // the inclusive prefix of the weights in sorted order, over the same tree on the first `live` places
  const int p0 = min(tid * c, live), p1 = min(tid * c + c, live);
  const double ex = hz_sorted_prefix(es, ix, p0, p1, sh, par);
  for (int k = 0; k < nq; ++k) {
    const double target = batch.level[k] * W;
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
  if (tid < nq) {
    int pos = min(min(sh.i[par][tid][0], sh.i[par][tid][1]), min(sh.i[par][tid][2], sh.i[par][tid][3]));
    if (pos >= live) pos = live - 1;  // rounding left no such row: the last row with weight
    q.qrow[out * nq + tid] = ix[pos];
    q.qval[out * nq + tid] = key[pos];
  }
}

}  // namespace

hipError_t mmt_launch_horizon(const HorizonBatch& b, int n, void* scratch, int64_t rows, int64_t per, int batch,
                              int samples, int steps, const double* logw, hipStream_t s) {
  HzScratch sc;
  sc.base = static_cast<char*>(scratch);
  sc.rows = rows;
  sc.cells = rows * steps;
  sc.per = per;
  hipLaunchKernelGGL(horizon_walk_kernel, dim3((unsigned)((rows + HZ_THREADS - 1) / HZ_THREADS), (unsigned)n),
                     dim3(HZ_THREADS), 0, s, b, sc, steps);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(horizon_reduce_kernel, dim3((unsigned)((int64_t)batch * steps), (unsigned)n), dim3(HZ_THREADS), 0, s,
                     b, sc, samples, steps, logw);
  return hipGetLastError();
}

extern "C" {

int64_t mmt_horizon_scratch_bytes(int32_t count, int32_t batch, int32_t samples, int32_t steps) {
  HzScratch sc;
  int64_t bytes;
  if (!hz_plan(count, batch, samples, steps, sc, bytes)) return -1;
  if (samples > HZ_MAX_S) return -1;
  return bytes;
}

int mmt_horizon_stats(void* stream, int32_t count, int32_t batch, int32_t samples, int32_t steps, const int32_t* V,
                      const int64_t* const* tok, const int64_t* tok_stride, const double* const* values,
                      const int32_t* is_percent, const int64_t* const* origin, const int64_t* origin_stride,
                      const double* logw, int32_t nq, const double* levels, int32_t nb, const double* const* barriers,
                      double* const* stats, double* const* qval, int32_t* const* qrow, double* const* hit,
                      double* const* ess, int32_t* const* live, void* scratch, int64_t scratch_bytes) {
  if (count < 0 || batch < 0 || steps < 0 || samples < 1) return MMT_ERR_INVALID;
  if ((int64_t)batch * samples > 0x7fffffff) return MMT_ERR_INVALID;
  if (nq < 0 || nq > MMT_HZ_MAX_Q || nb < 0 || nb > MMT_HZ_MAX_B) return MMT_ERR_INVALID;
  if (nq > 0 && !levels) return MMT_ERR_INVALID;
  for (int k = 0; k < nq; ++k)
    if (!(levels[k] > 0.0 && levels[k] < 1.0)) return MMT_ERR_INVALID;
  if (count == 0) return MMT_OK;
  if (!V || !tok || !tok_stride || !values || !stats || (nq > 0 && (!qval || !qrow)) || (nb > 0 && (!hit || !barriers)))
    return MMT_ERR_INVALID;
  const bool work = batch > 0 && steps > 0;
  for (int p = 0; p < count; ++p) {
    const bool pct = is_percent && is_percent[p];
    if (V[p] < 1 || tok_stride[p] < steps) return MMT_ERR_INVALID;
    if (!pct && (!origin || !origin_stride)) return MMT_ERR_INVALID;
    if (nb > 0) {
      if (!barriers[p]) return MMT_ERR_INVALID;
      for (int k = 0; k < nb; ++k) {
        const double u = barriers[p][k];
        if (!(std::fabs(u) < INFINITY) || u == 0.0) return MMT_ERR_INVALID;
      }
    }
    if (work) {
      if (!tok[p] || !values[p] || !stats[p] || (!pct && !origin[p])) return MMT_ERR_INVALID;
      if (nq > 0 && (!qval[p] || !qrow[p])) return MMT_ERR_INVALID;
      if (nb > 0 && !hit[p]) return MMT_ERR_INVALID;
    }
  }
  HzScratch sc;
  int64_t bytes;
  if (!hz_plan(count, batch, samples, steps, sc, bytes)) return MMT_ERR_INVALID;
  if (work && (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < bytes)) return MMT_ERR_INVALID;
  for (int p = 0; p < count; ++p)
    if (V[p] > SAMPLE_MAX_V) return MMT_ERR_UNSUPPORTED;
  if (samples > HZ_MAX_S) return MMT_ERR_UNSUPPORTED;
  if ((int64_t)batch * steps > 0x7fffffff) return MMT_ERR_UNSUPPORTED;
  if (!work) return MMT_OK;

  for (int p0 = 0; p0 < count; p0 += MMT_MAX_GROUP) {
    HorizonBatch hb;
    const int n = count - p0 < MMT_MAX_GROUP ? count - p0 : MMT_MAX_GROUP;
    for (int k = 0; k < MMT_MAX_GROUP; ++k) {
      const int p = p0 + (k < n ? k : 0);
      HorizonProblem& q = hb.p[k];
      const bool pct = is_percent && is_percent[p];
      q.tok = tok[p];
      q.tok_stride = tok_stride[p];
      q.values = values[p];
      q.origin = pct ? nullptr : origin[p];
      q.origin_stride = pct ? 0 : origin_stride[p];
      q.stats = stats[p];
      q.qval = nq > 0 ? qval[p] : nullptr;
      q.qrow = nq > 0 ? qrow[p] : nullptr;
      q.hit = nb > 0 ? hit[p] : nullptr;
      q.ess = ess ? ess[p] : nullptr;
      q.live = live ? live[p] : nullptr;
      for (int i = 0; i < MMT_HZ_MAX_B; ++i) q.barrier[i] = i < nb ? barriers[p][i] : 1.0;
      q.V = V[p];
      q.is_percent = pct ? 1 : 0;
      q.index = p;
    }
    for (int k = 0; k < MMT_HZ_MAX_Q; ++k) hb.level[k] = k < nq ? levels[k] : 0.5;
    hb.nq = nq;
    hb.nb = nb;
    if (mmt_launch_horizon(hb, n, scratch, sc.rows, sc.per, batch, samples, steps, logw, (hipStream_t)stream) !=
        hipSuccess)
      return MMT_ERR_HIP;
  }
  return MMT_OK;
}

}  // extern "C"
