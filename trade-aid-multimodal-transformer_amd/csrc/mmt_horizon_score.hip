// Scores of horizon forecasts against what happened (mmt.h: mmt_horizon_score): per (prompt, step) the CRPS and the
// mid-PIT of the weighted sample of cumulative changes at the realised change, the pointwise scores of the forecast
// mmt_horizon_stats made from the same paths (error of the mean, mass on the realised signs, pinball loss per quantile,
// Brier score per barrier), and per step the tables that a backtest accumulates over its evaluation batches.
//
// Three launches per chunk of 8 problems:
//   walk    grid (ceil((batch samples + batch) / 256), problems), 256 threads: mmt_horizon_stats' walk (the same
//           device function, mmt_horizon_dev.h) over the path rows and, behind them, the realised row of every prompt:
//           x, hi, lo (fp64) and d (int8) step-major in the scratch, plus the row's dead flag.
//   reduce  grid (prompts x steps, problems), 256 threads: the weights of the prompt in LDS (rule 2), W and the two PIT
//           masses in row order over the chunk tree, the bitonic sort of (x, s) in LDS, the prefix of the weights in
//           sorted order over the same tree, and the CRPS terms of the gaps, a thread summing the gaps above its own
//           places serially and the tree the thread totals. Thread 0 writes the record, threads k < nq / nb the
//           pinball / Brier entries.
//   tables  grid (steps, problems), 256 threads: thread t owns one cell of agg (10), aggq (2 nq), aggb (3 nb) or pit
//           (bins) and sums it serially over b ascending from the records and the forecast; one store, or with
//           `accumulate` one load, one addition and one store.
// LDS of reduce at the cap of 4096 rows: fp64 keys 32 KiB + 16-bit indices 8 KiB + fp32 weights 16 KiB = 56 KiB, and
// under 2 KiB of reduction slots: mmt_horizon_stats' footprint, inside the 64 KiB of a static allocation.
// No float atomics, no data-dependent order of a sum: bit-identical run to run; a (prompt, step, problem) reads its own
// rows only, a table cell its own step's records only.
//
// Every rule is one IEEE operation per line: floating-point contraction is off for this file (the header turns it off
// for its own code), or the compiler fuses a product into the sum that follows it and the records lose their bits
// against the rule.
#include <cmath>

#include "mmt.h"
#include "mmt_common.h"
#include "mmt_kernels.h"
#include "mmt_horizon_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int HS_REC = 8;        // fields of a record
constexpr int HS_AGG = 10;       // cells of agg per step
constexpr int HS_MAX_BINS = 64;  // 10 + 2 * 16 + 3 * 8 + 64 = 130 cells at the most: one block of 256 threads

// walk over batch * samples + batch rows, then the records of a problem whose caller passed none
bool hs_plan(int32_t count, int32_t batch, int32_t samples, int32_t steps, HzScratch& sc, int64_t& walk, int64_t& bytes) {
  if (count < 0 || batch < 0 || steps < 0 || samples < 1) return false;
  if ((int64_t)batch * samples > 0x7fffffff || (int64_t)batch * samples + batch > 0x7fffffff) return false;
  sc.rows = (int64_t)batch * samples + batch;
  sc.cells = sc.rows * steps;
  if (sc.cells > ((int64_t)1 << 44)) return false;  // 25 bytes a cell: far past any device, and no overflow below
  walk = sc.walk_bytes();
  sc.per = walk + (int64_t)HS_REC * 8 * batch * steps;
  if (count > 0 && sc.per > (int64_t)0x7fffffffffffll / count) return false;
  bytes = sc.per * count;
  return true;
}

__global__ __launch_bounds__(HZ_THREADS) void score_walk_kernel(HorizonScoreBatch batch, HzScratch sc, int64_t paths,
                                                                int steps) {
  const HorizonScoreProblem& q = batch.p[blockIdx.y];
  const int64_t r = (int64_t)blockIdx.x * HZ_THREADS + threadIdx.x;
  if (r >= sc.rows) return;
  const int64_t* tk;
  const int64_t* org = nullptr;
  if (r < paths) {
    tk = q.tok + r * q.tok_stride;
    if (!q.is_percent) org = q.origin + r * q.origin_stride;
  } else {
    const int64_t b = r - paths;
    tk = q.real + b * q.real_stride;
    if (!q.is_percent) org = q.real_origin + b * q.real_origin_stride;
  }
  const bool ok = hz_walk_row(tk, org, q.values, q.V, q.is_percent, steps, sc.x(q.index) + r, sc.hi(q.index) + r,
                              sc.lo(q.index) + r, sc.d(q.index) + r, sc.rows);
  sc.dead(q.index)[r] = ok ? 0 : 1;
}

__global__ __launch_bounds__(HZ_THREADS) void score_reduce_kernel(HorizonScoreBatch batch, HzScratch sc, int B, int S,
                                                                  int steps, const double* __restrict__ logw) {
  __shared__ double key[HZ_MAX_S];
  __shared__ float es[HZ_MAX_S];
  __shared__ uint16_t ix[HZ_MAX_S];
  __shared__ HzShared sh;
  const HorizonScoreProblem& q = batch.p[blockIdx.y];
  const int tid = threadIdx.x;
  const int nq = batch.nq, nb = batch.nb;
  const int b = blockIdx.x / steps, j = blockIdx.x % steps;
  const int64_t r0 = (int64_t)b * S, rr = (int64_t)B * S + b, out = (int64_t)b * steps + j;
  const int64_t cell = (int64_t)j * sc.rows + r0, rcell = (int64_t)j * sc.rows + rr;
  const double* __restrict__ xs = sc.x(q.index) + cell;
  const int32_t* __restrict__ dead = sc.dead(q.index) + r0;
  double* rec = q.rec + out * HS_REC;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  int par = 0;

  // rule 1's verdict on the realised row, then rule 2 (both branches are uniform over the block)
  const bool rdead = sc.dead(q.index)[rr] != 0;
  const double mx = rdead ? -INFINITY : hz_weight_max(logw, dead, r0, S, sh, par);
  if (mx == -INFINITY) {  // a dead realised row or no live path
    if (tid < HS_REC) rec[tid] = nan;
    if (tid < nq) q.pin[out * nq + tid] = nan;
    if (tid < nb) q.bs[out * nb + tid] = nan;
    return;
  }
  hz_weight_fill(logw, dead, r0, S, mx, es);
  const double xr = sc.x(q.index)[rcell], hr = sc.hi(q.index)[rcell], lr = sc.lo(q.index)[rcell];
  const int dr = sc.d(q.index)[rcell];

  // W and the PIT masses in row order over the chunk tree
  const int c = ((S + HZ_THREADS - 1) / HZ_THREADS) | 1;
  const int i0 = min(tid * c, S), i1 = min(tid * c + c, S);
  double v[3] = {0.0, 0.0, 0.0};
  int live = 0;
  for (int i = i0; i < i1; ++i) {
    const float e = es[i];
    if (!(e > 0.f)) continue;  // a dead row's cells were never written
    const double w = (double)e, x = xs[i];
    ++live;
    v[0] += w;
    v[1] += x < xr ? w : 0.0;
    v[2] += x == xr ? w : 0.0;
  }
  hz_sums(v, 3, sh, par);
  live = hz_count(live, sh, par);
  const double W = v[0];

  // rule 3: the gaps between neighbouring places of the order (x, s), place order over the tree
  hz_sort(xs, es, S, key, ix);
  const int p0 = min(tid * c, live), p1 = min(tid * c + c, live);
  double p = hz_sorted_prefix(es, ix, p0, p1, sh, par);
  double gap[1] = {0.0};
  for (int i = p0; i < p1; ++i) {
    p += (double)es[ix[i]];
    if (i + 1 >= live) break;  // the last place has no gap above it
    const double lo_x = key[i], hi_x = key[i + 1];
    const double s = fmin(hi_x, fmax(lo_x, xr));
    const double F = p / W;
    const double F2 = F * F;
    const double G = 1.0 - F;
    const double G2 = G * G;
    const double below = (s - lo_x) * F2;
    const double above = (hi_x - s) * G2;
    gap[0] += below + above;
  }
  hz_sums(gap, 1, sh, par);

  const double* __restrict__ st = q.stats + out * 12;
  if (tid == 0) {
    const double x1 = key[0], xn = key[live - 1];
    const double tail = xr < x1 ? x1 - xr : xr > xn ? xr - xn : 0.0;
    const double half = 0.5 * v[2];
    rec[0] = xr;
    rec[1] = gap[0] + tail;
    rec[2] = (v[1] + half) / W;
    rec[3] = st[0] - xr;
    rec[4] = st[3 + hz_sign(xr)];
    rec[5] = st[6 + dr];
    rec[6] = hr;
    rec[7] = lr;
  }
  if (tid < nq) {
    const double qv = q.qval[out * nq + tid];
    const double diff = xr - qv;
    const double m = batch.level[tid] - (xr < qv ? 1.0 : 0.0);
    q.pin[out * nq + tid] = diff * m;
  }
#pragma unroll
  for (int k = 0; k < MMT_HZ_MAX_B; ++k)
    if (tid == k && k < nb) {
      const double u = q.barrier[k];
      const double o = (u > 0.0 ? hr >= u : lr <= u) ? 1.0 : 0.0;
      const double e = q.hit[out * nb + k] - o;
      q.bs[out * nb + k] = e * e;
    }
}

// the index of the largest of three, the lowest on ties
__device__ __forceinline__ int hs_argmax3(const double* m) {
  int k = 0;
  if (m[1] > m[k]) k = 1;
  if (m[2] > m[k]) k = 2;
  return k;
}

__global__ __launch_bounds__(HZ_THREADS) void score_tables_kernel(HorizonScoreBatch batch, HzScratch sc, int B, int S,
                                                                  int steps, int bins, int accumulate) {
  const HorizonScoreProblem& q = batch.p[blockIdx.y];
  const int nq = batch.nq, nb = batch.nb, j = blockIdx.x;
  int t = threadIdx.x;
  // the cell of this thread: kind 0 agg, 1 aggq, 2 aggb, 3 pit; k the level / barrier / bin, f the field
  int kind, k = 0, f = 0;
  double* dst;
  if (t < HS_AGG) {
    kind = 0, f = t, dst = q.agg + (int64_t)j * HS_AGG + t;
  } else if ((t -= HS_AGG) < 2 * nq) {
    kind = 1, k = t >> 1, f = t & 1, dst = q.aggq + (int64_t)j * 2 * nq + t;
  } else if ((t -= 2 * nq) < 3 * nb) {
    kind = 2, k = t / 3, f = t % 3, dst = q.aggb + (int64_t)j * 3 * nb + t;
  } else if ((t -= 3 * nb) < bins) {
    kind = 3, k = t, dst = q.pit + (int64_t)j * bins + t;
  } else {
    return;
  }
  double u = 1.0;
#pragma unroll
  for (int i = 0; i < MMT_HZ_MAX_B; ++i)
    if (kind == 2 && i == k) u = q.barrier[i];
  const int8_t* __restrict__ dstar = sc.d(q.index) + (int64_t)j * sc.rows + (int64_t)B * S;
  double sum = 0.0;
  for (int b = 0; b < B; ++b) {
    const int64_t out = (int64_t)b * steps + j;
    const double* __restrict__ rec = q.rec + out * HS_REC;
    const double xr = rec[0];
    if (xr != xr) continue;  // a dead (b, j) enters no table
    const double* __restrict__ st = q.stats + out * 12;
    double add = 0.0;
    if (kind == 0) {
      switch (f) {
        case 0: add = 1.0; break;
        case 1: add = rec[1]; break;
        case 2: add = fabs(xr); break;
        case 3: add = fabs(rec[3]); break;
        case 4: add = rec[3] * rec[3]; break;
        case 5: add = rec[4]; break;
        case 6: add = hs_argmax3(st + 2) == 1 + hz_sign(xr) ? 1.0 : 0.0; break;
        case 7: add = rec[5]; break;
        case 8: add = hs_argmax3(st + 5) == 1 + dstar[b] ? 1.0 : 0.0; break;
        default: add = st[1]; break;
      }
    } else if (kind == 1) {
      add = f == 0 ? q.pin[out * nq + k] : (xr <= q.qval[out * nq + k] ? 1.0 : 0.0);
    } else if (kind == 2) {
      const double o = (u > 0.0 ? rec[6] >= u : rec[7] <= u) ? 1.0 : 0.0;
      add = f == 0 ? q.bs[out * nb + k] : f == 1 ? q.hit[out * nb + k] : o;
    } else {
      const double scaled = rec[2] * (double)bins;
      const int bin = min(bins - 1, (int)floor(scaled));
      add = bin == k ? 1.0 : 0.0;
    }
    sum += add;
  }
  *dst = accumulate ? *dst + sum : sum;
}

}  // namespace

hipError_t mmt_launch_horizon_score(const HorizonScoreBatch& b, int n, void* scratch, int64_t per, int batch,
                                    int samples, int steps, int bins, int accumulate, const double* logw,
                                    hipStream_t s) {
  HzScratch sc;
  sc.base = static_cast<char*>(scratch);
  sc.rows = (int64_t)batch * samples + batch;
  sc.cells = sc.rows * steps;
  sc.per = per;
  hipLaunchKernelGGL(score_walk_kernel, dim3((unsigned)((sc.rows + HZ_THREADS - 1) / HZ_THREADS), (unsigned)n),
                     dim3(HZ_THREADS), 0, s, b, sc, (int64_t)batch * samples, steps);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)((int64_t)batch * steps), (unsigned)n), dim3(HZ_THREADS), 0, s,
                     b, sc, batch, samples, steps, logw);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(score_tables_kernel, dim3((unsigned)steps, (unsigned)n), dim3(HZ_THREADS), 0, s, b, sc, batch,
                     samples, steps, bins, accumulate);
  return hipGetLastError();
}

extern "C" {

int64_t mmt_horizon_score_scratch_bytes(int32_t count, int32_t batch, int32_t samples, int32_t steps) {
  HzScratch sc;
  int64_t walk, bytes;
  if (!hs_plan(count, batch, samples, steps, sc, walk, bytes)) return -1;
  if (samples > HZ_MAX_S) return -1;
  return bytes;
}

int mmt_horizon_score(void* stream, int32_t count, int32_t batch, int32_t samples, int32_t steps, const int32_t* V,
                      const int64_t* const* tok, const int64_t* tok_stride, const double* const* values,
                      const int32_t* is_percent, const int64_t* const* origin, const int64_t* origin_stride,
                      const int64_t* const* real, const int64_t* real_stride, const int64_t* const* real_origin,
                      const int64_t* real_origin_stride, const double* logw, int32_t nq, const double* levels,
                      int32_t nb, const double* const* barriers, const double* const* stats,
                      const double* const* qval, const double* const* hit, int32_t bins, int32_t accumulate,
                      double* const* sc_out, double* const* pin, double* const* bs, double* const* agg,
                      double* const* aggq, double* const* aggb, double* const* pit, void* scratch,
                      int64_t scratch_bytes) {
  if (count < 0 || batch < 0 || steps < 0 || samples < 1) return MMT_ERR_INVALID;
  if ((int64_t)batch * samples + batch > 0x7fffffff) return MMT_ERR_INVALID;
  if (nq < 0 || nq > MMT_HZ_MAX_Q || nb < 0 || nb > MMT_HZ_MAX_B) return MMT_ERR_INVALID;
  if (bins < 1 || bins > HS_MAX_BINS) return MMT_ERR_INVALID;
  if (nq > 0 && !levels) return MMT_ERR_INVALID;
  for (int k = 0; k < nq; ++k)
    if (!(levels[k] > 0.0 && levels[k] < 1.0)) return MMT_ERR_INVALID;
  if (count == 0) return MMT_OK;
  if (!V || !tok || !tok_stride || !values || !real || !real_stride || !stats || !agg || !pit) return MMT_ERR_INVALID;
  if (nq > 0 && (!qval || !pin || !aggq)) return MMT_ERR_INVALID;
  if (nb > 0 && (!hit || !bs || !aggb || !barriers)) return MMT_ERR_INVALID;
  const bool work = batch > 0 && steps > 0;
  for (int p = 0; p < count; ++p) {
    const bool pct = is_percent && is_percent[p];
    if (V[p] < 1 || tok_stride[p] < steps || real_stride[p] < steps) return MMT_ERR_INVALID;
    if (!pct && (!origin || !origin_stride || !real_origin || !real_origin_stride)) return MMT_ERR_INVALID;
    if (nb > 0) {
      if (!barriers[p]) return MMT_ERR_INVALID;
      for (int k = 0; k < nb; ++k) {
        const double u = barriers[p][k];
        if (!(std::fabs(u) < INFINITY) || u == 0.0) return MMT_ERR_INVALID;
      }
    }
    if (work) {
      if (!tok[p] || !values[p] || !real[p] || !stats[p] || !agg[p] || !pit[p]) return MMT_ERR_INVALID;
      if (!pct && (!origin[p] || !real_origin[p])) return MMT_ERR_INVALID;
      if (nq > 0 && (!qval[p] || !pin[p] || !aggq[p])) return MMT_ERR_INVALID;
      if (nb > 0 && (!hit[p] || !bs[p] || !aggb[p])) return MMT_ERR_INVALID;
    }
  }
  HzScratch sc;
  int64_t walk, bytes;
  if (!hs_plan(count, batch, samples, steps, sc, walk, bytes)) return MMT_ERR_INVALID;
  if (work && (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < bytes)) return MMT_ERR_INVALID;
  for (int p = 0; p < count; ++p)
    if (V[p] > SAMPLE_MAX_V) return MMT_ERR_UNSUPPORTED;
  if (samples > HZ_MAX_S) return MMT_ERR_UNSUPPORTED;
  if ((int64_t)batch * steps > 0x7fffffff) return MMT_ERR_UNSUPPORTED;
  if (!work) return MMT_OK;

  for (int p0 = 0; p0 < count; p0 += MMT_MAX_GROUP) {
    HorizonScoreBatch hb;
    const int n = count - p0 < MMT_MAX_GROUP ? count - p0 : MMT_MAX_GROUP;
    for (int k = 0; k < MMT_MAX_GROUP; ++k) {
      const int p = p0 + (k < n ? k : 0);
      HorizonScoreProblem& q = hb.p[k];
      const bool pct = is_percent && is_percent[p];
      q.tok = tok[p];
      q.tok_stride = tok_stride[p];
      q.real = real[p];
      q.real_stride = real_stride[p];
      q.values = values[p];
      q.origin = pct ? nullptr : origin[p];
      q.origin_stride = pct ? 0 : origin_stride[p];
      q.real_origin = pct ? nullptr : real_origin[p];
      q.real_origin_stride = pct ? 0 : real_origin_stride[p];
      q.stats = stats[p];
      q.qval = nq > 0 ? qval[p] : nullptr;
      q.hit = nb > 0 ? hit[p] : nullptr;
      q.rec = sc_out && sc_out[p] ? sc_out[p]
                                  : reinterpret_cast<double*>(static_cast<char*>(scratch) + p * sc.per + walk);
      q.pin = nq > 0 ? pin[p] : nullptr;
      q.bs = nb > 0 ? bs[p] : nullptr;
      q.agg = agg[p];
      q.aggq = nq > 0 ? aggq[p] : nullptr;
      q.aggb = nb > 0 ? aggb[p] : nullptr;
      q.pit = pit[p];
      for (int i = 0; i < MMT_HZ_MAX_B; ++i) q.barrier[i] = i < nb ? barriers[p][i] : 1.0;
      q.V = V[p];
      q.is_percent = pct ? 1 : 0;
      q.index = p;
    }
    for (int k = 0; k < MMT_HZ_MAX_Q; ++k) hb.level[k] = k < nq ? levels[k] : 0.5;
    hb.nq = nq;
    hb.nb = nb;
    if (mmt_launch_horizon_score(hb, n, scratch, sc.per, batch, samples, steps, bins, accumulate, logw,
                                 (hipStream_t)stream) != hipSuccess)
      return MMT_ERR_HIP;
  }
  return MMT_OK;
}

}  // extern "C"
