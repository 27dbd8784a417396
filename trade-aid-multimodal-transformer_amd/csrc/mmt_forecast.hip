// Forecast distributions of rollouts (mmt.h: mmt_forecast_multi, mmt_pmf_stats): per generated step and prompt the
// evidence-weighted mixture of the laws the prompt's paths draw their next token from, and its summaries.
//
// mmt_forecast_multi is two launches without weights and three with them:
//   law      grid (rows, problems), 256 threads: the sampler's own front (row_law, mmt_sample_dev.h) leaves
//            (m, K, S_r) of every row in the scratch; S_r == 0 marks a row with no finite logit. A greedy problem
//            leaves the token (the lowest index among the maxima) in K and S_r = 1.
//   weights  grid (prompts, problems), 256 threads, only with weights: mmt_resample's rules 1 - 2 over the rows that
//            are not dead in the problem, the a_s and the fp32 weights in LDS (48 KiB at 4096 paths), W and Q over the
//            sampler's chunk tree. Leaves the weights and (W, ESS, live) in the scratch, and on request the a_s (before
//            any problem's dead rows are cut) for a caller that carries them from step to step.
//   mix      grid (prompts x column chunks, problems), 1024 threads: a workgroup owns 64 consecutive columns of one
//            prompt, lane l column l of the chunk; wave w of 16 walks the rows [w per, w per + per), per =
//            ceil(samples / 16), in order, one fp64 fused multiply-add per row; the sixteen partial sums are added
//            left to right, divided by W and rounded to fp32 once. Without weights the workgroup counts the prompt's live
//            rows itself (an integer, so any order gives it). A wave's loads are 256 contiguous bytes of one row.
// No float atomics and no data-dependent order: a launch is bit-identical run to run, and a prompt's bits depend on
// its own rows and on `samples` only.
//
// mmt_pmf_stats: grid (rows, problems), 256 threads, a pmf row per workgroup: fp64 sums in vocabulary order over
// the sampler's chunk tree (thread t owns [t c, t c + c), c = ceil(V / 256) | 1; serial sum, shift scan over the
// lanes, the four wave totals left to right); a quantile is found on the prefix sums of that tree as the sampler
// finds its token.
#include "mmt.h"
#include "mmt_common.h"
#include "mmt_kernels.h"
#include "mmt_sample_dev.h"

namespace {

constexpr int FC_MAX_S = 4096;  // with weights: the S weights of a prompt stay in LDS (mmt_resample's cap)
constexpr int MIX_WAVES = 16;
constexpr int MIX_THREADS = MIX_WAVES * MMT_WAVE;
constexpr int MIX_COLS = MMT_WAVE;

template <bool ONCHIP>
__global__ __launch_bounds__(SAMPLE_THREADS) void forecast_law_kernel(ForecastBatch batch, int64_t rows,
                                                                      ForecastRowInfo* __restrict__ info) {
  __shared__ float zs[ONCHIP ? SAMPLE_ONCHIP : 1];
  __shared__ SampleShared sh;
  const ForecastProblem& q = batch.p[blockIdx.y];
  const int tid = threadIdx.x, V = q.V;
  const int64_t r = blockIdx.x;
  const float* row = q.logits + r * q.row_stride;
  const float inv_t = q.inv_t;
  int par = 0;
  auto zat = [&](int i) -> float { return ONCHIP ? zs[i] : scaled_logit(row, i, inv_t); };
  const RowLaw law = row_law<ONCHIP>(zat, zs, row, V, inv_t, q.greedy, q.top_k, q.top_p, sh, par);
  ForecastRowInfo* out = info + (int64_t)q.index * rows + r;
  if (law.m == -INFINITY) {  // no finite logit: no law (uniform branch)
    if (tid == 0) *out = ForecastRowInfo{0.0, law.m, 0u};
    return;
  }
  if (!q.greedy) {
    if (tid == 0) *out = ForecastRowInfo{law.rs.S, law.m, law.K};
    return;
  }
  // greedy: a point mass on the lowest index among the maxima. A thread's first hit is its lowest (ascending walk).
  int first = V;
  for (int i = tid; i < V; i += SAMPLE_THREADS)
    if (zat(i) == law.m) { first = i; break; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  if ((tid & 63) == 0) sh.i[par][tid >> 6] = first;
  __syncthreads();
  if (tid == 0) {
    first = min(min(sh.i[par][0], sh.i[par][1]), min(sh.i[par][2], sh.i[par][3]));
    *out = ForecastRowInfo{1.0, law.m, (uint32_t)first};
  }
}

// mmt_resample's rules 1 - 2 for prompt b = blockIdx.x in problem p = blockIdx.y; rows dead in p take no part.
__global__ __launch_bounds__(SAMPLE_THREADS) void forecast_weights_kernel(
    ForecastWeights in, int batch, int S, int j0, int j1, const double* __restrict__ logw,
    double* __restrict__ logw_out, const ForecastRowInfo* __restrict__ info, float* __restrict__ omega,
    ForecastPromptInfo* __restrict__ pinfo) {
  __shared__ double ps[FC_MAX_S];
  __shared__ float es[FC_MAX_S];
  __shared__ double shd[3][SAMPLE_WAVES];
  __shared__ int shi[SAMPLE_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, p = blockIdx.y;
  const int64_t r0 = (int64_t)b * S;
  const int64_t base = (int64_t)p * batch * S + r0;

  double mx = -INFINITY;
  for (int s = tid; s < S; s += SAMPLE_THREADS) {
    const int64_t r = r0 + s;
    double a = logw ? logw[r] : 0.0;
    if (a != a) a = -INFINITY;
    for (int j = j0; j < j1; ++j)
      for (int g = 0; g < in.count; ++g) {
        double t = (double)in.lp[g][r * in.stride[g] + j];
        if (t != t) t = -INFINITY;
        a += t;
      }
    if (a != a) a = -INFINITY;
    if (logw_out && p == 0) logw_out[r] = a;  // rule 1's sum, the same in every problem: problem 0 writes it
    if (!(info[base + s].S > 0.0)) a = -INFINITY;  // dead in this problem
    ps[s] = a;
    mx = fmax(mx, a);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) shd[0][wave] = mx;
  __syncthreads();
  mx = fmax(fmax(shd[0][0], shd[0][1]), fmax(shd[0][2], shd[0][3]));

  if (mx == -INFINITY) {  // no live path (uniform branch)
    for (int s = tid; s < S; s += SAMPLE_THREADS) omega[base + s] = 0.f;
    if (tid == 0) pinfo[(int64_t)p * batch + b] = ForecastPromptInfo{0.0, 0.0, 0, 0};
    return;
  }
  for (int s = tid; s < S; s += SAMPLE_THREADS) {  // every thread reads back its own ps entries
    const double a = ps[s];
    float e = 0.f;
    if (a != -INFINITY) {
      const float d = (float)(a - mx);
      e = d == 0.f ? 1.0f : expf(d);
    }
    es[s] = e;
    omega[base + s] = e;
  }
  __syncthreads();
  const int c = ((S + SAMPLE_THREADS - 1) / SAMPLE_THREADS) | 1;
  const int i0 = min(tid * c, S), i1 = min(tid * c + c, S);
  double totW = 0.0, totQ = 0.0;
  int live = 0;
  for (int i = i0; i < i1; ++i) {
    const double w = (double)es[i];
    totW += w;
    totQ += w * w;  // the product of two fp32 values is exact in fp64
    live += es[i] > 0.f ? 1 : 0;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double nW = __shfl_up(totW, o, 64), nQ = __shfl_up(totQ, o, 64);
    if (lane >= o) { totW += nW; totQ += nQ; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) live += __shfl_xor(live, o, 64);
  if (lane == 63) { shd[1][wave] = totW; shd[2][wave] = totQ; }
  if (lane == 0) shi[wave] = live;
  __syncthreads();
  if (tid == 0) {
    const double W = ((shd[1][0] + shd[1][1]) + shd[1][2]) + shd[1][3];
    const double Q = ((shd[2][0] + shd[2][1]) + shd[2][2]) + shd[2][3];
    pinfo[(int64_t)p * batch + b] = ForecastPromptInfo{W, W * W / Q, shi[0] + shi[1] + shi[2] + shi[3], 0};
  }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(MIX_THREADS) void forecast_mix_kernel(
    ForecastBatch batch, int nb, int S, int nchunks, const ForecastRowInfo* __restrict__ info,
    const float* __restrict__ omega, const ForecastPromptInfo* __restrict__ pinfo) {
  __shared__ double part[MIX_WAVES][MIX_COLS];
  __shared__ int cnt[MIX_WAVES];
  const ForecastProblem& q = batch.p[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
  const int V = q.V;
  if (chunk * MIX_COLS >= V) return;  // a shorter row than the launch's longest (uniform)
  const int64_t r0 = (int64_t)b * S;
  const int64_t base = (int64_t)q.index * nb * S + r0;
  const ForecastRowInfo* ri = info + base;

  double W, ess;
  int live;
  if (WEIGHTED) {
    const ForecastPromptInfo pi = pinfo[(int64_t)q.index * nb + b];
    W = pi.W;
    ess = pi.ess;
    live = pi.live;
  } else {  // every live row weighs 1: W = Q = their number
    int n = 0;
    for (int s = tid; s < S; s += MIX_THREADS) n += ri[s].S > 0.0 ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) cnt[wave] = n;
    __syncthreads();
    n = 0;
#pragma unroll
    for (int w = 0; w < MIX_WAVES; ++w) n += cnt[w];
    live = n;
    W = ess = (double)n;
  }
  if (chunk == 0 && tid == 0) {
    if (q.ess) q.ess[b] = ess;
    if (q.live) q.live[b] = live;
  }
  const int col = chunk * MIX_COLS + lane;
  float* out = q.pmf + (int64_t)b * q.pmf_stride + col;
  if (!(W > 0.0)) {  // no live path: a zero row (uniform branch)
    if (wave == 0 && col < V) *out = 0.f;
    return;
  }

  const int per = (S + MIX_WAVES - 1) / MIX_WAVES;
  const int s0 = min((int64_t)wave * per, (int64_t)S), s1 = min((int64_t)wave * per + per, (int64_t)S);
  const float inv_t = q.inv_t;
  const int greedy = q.greedy;
  // No branch in the loop, so the loads of several rows are in flight at once (the walk waits for memory, not for
  // arithmetic): a dead or weightless row takes c = 0, and its term e * 0 leaves acc as it is (e is always finite: a
  // row without a finite logit gives e = 1); a lane past the row's end reads the last column and writes nothing.
  const int colc = col < V ? col : V - 1;
  const float* lg = q.logits + r0 * q.row_stride + colc;
  double acc = 0.0;
#pragma unroll 8
  for (int s = s0; s < s1; ++s) {
    const ForecastRowInfo law = ri[s];  // wave-uniform
    const float om = WEIGHTED ? omega[base + s] : 1.0f;
    const double c = (law.S > 0.0 && om > 0.f) ? (double)om / law.S : 0.0;
    const float z = scaled_logit(lg + (int64_t)s * q.row_stride, 0, inv_t);
    const float e = greedy ? ((uint32_t)colc == law.K ? 1.0f : 0.0f) : (okey(z) >= law.K ? weight(z, law.m) : 0.0f);
    acc = fma((double)e, c, acc);
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && col < V) {
    double t = part[0][lane];
#pragma unroll
    for (int w = 1; w < MIX_WAVES; ++w) t += part[w][lane];
    *out = (float)(t / W);
  }
}

// ---- mmt_pmf_stats ----

struct StatsShared {
  double d[2][SAMPLE_WAVES];
  int i[2][SAMPLE_WAVES];
  float f[SAMPLE_WAVES];
};
// the chunk tree: a thread's serial total in, the row total out, and the thread's exclusive prefix
__device__ __forceinline__ double stats_scan(double tot, double& ex, StatsShared& sh, int& par) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double inc = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = 0.0;
  if (lane == 63) sh.d[par][wave] = inc;
  __syncthreads();
  const double w0 = sh.d[par][0], w1 = sh.d[par][1], w2 = sh.d[par][2], w3 = sh.d[par][3];
  par ^= 1;
  ex += wave == 0 ? 0.0 : wave == 1 ? w0 : wave == 2 ? (w0 + w1) : ((w0 + w1) + w2);
  return ((w0 + w1) + w2) + w3;
}
__device__ __forceinline__ double stats_sum(double tot, StatsShared& sh, int& par) {
  double ex;
  return stats_scan(tot, ex, sh, par);
}
// block minimum (MIN) or maximum of an int
template <bool MIN>
__device__ __forceinline__ int stats_ext(int v, StatsShared& sh, int& par) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int n = __shfl_xor(v, o, 64);
    v = MIN ? min(v, n) : max(v, n);
  }
  if ((threadIdx.x & 63) == 0) sh.i[par][threadIdx.x >> 6] = v;
  __syncthreads();
  const int a = sh.i[par][0], b = sh.i[par][1], c = sh.i[par][2], d = sh.i[par][3];
  par ^= 1;
  return MIN ? min(min(a, b), min(c, d)) : max(max(a, b), max(c, d));
}

__global__ __launch_bounds__(SAMPLE_THREADS) void pmf_stats_kernel(PmfStatsBatch batch) {
  __shared__ StatsShared sh;
  const PmfStatsProblem& q = batch.p[blockIdx.y];
  const int tid = threadIdx.x, V = q.V, nq = batch.nq;
  const int64_t r = blockIdx.x;
  const float* row = q.pmf + r * q.stride;
  double* st = q.stats + r * 8;
  int32_t* qt = q.qtok + r * nq;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  int par = 0;
  const int c = ((V + SAMPLE_THREADS - 1) / SAMPLE_THREADS) | 1;
  const int64_t i0l = (int64_t)tid * c;
  const int i0 = i0l < V ? (int)i0l : V, i1 = i0l + c < V ? (int)(i0l + c) : V;
  // an entry that is not > 0 (a zero, a negative, a NaN) holds no mass
  auto at = [&](int i) -> double { const float x = row[i]; return x > 0.f ? (double)x : 0.0; };

  double tot = 0.0;
  float fmx = 0.f;
  int lastpos = -1;
  for (int i = i0; i < i1; ++i) {
    const double x = at(i);
    tot += x;
    if (x > 0.0) { lastpos = i; fmx = fmaxf(fmx, row[i]); }
  }
  double ex;
  const double T = stats_scan(tot, ex, sh, par);
  if (!(T > 0.0)) {  // no mass (uniform branch)
    if (tid == 0) {
      st[0] = T;
      for (int k = 1; k < 8; ++k) st[k] = nan;
    }
    for (int k = tid; k < nq; k += SAMPLE_THREADS) qt[k] = -1;
    return;
  }
  lastpos = stats_ext<false>(lastpos, sh, par);
  fmx = warp_max(fmx);
  if ((tid & 63) == 0) sh.f[tid >> 6] = fmx;  // read after the barriers of the sums below

  const double* val = q.values;
  // the direction classes: -1 / 0 / +1 of the value itself (percent) or of value - value[origin]; none without
  // values or with an origin outside the vocabulary
  bool dir = val != nullptr;
  double vo = 0.0;
  if (dir && !q.is_percent) {
    const int64_t o = q.origin ? q.origin[r * q.origin_stride] : -1;
    dir = o >= 0 && o < V;
    if (dir) vo = val[o];
  }
  double ent = 0.0, mean = 0.0, dn = 0.0, fl = 0.0, up = 0.0;
  for (int i = i0; i < i1; ++i) {
    const double x = at(i);
    if (!(x > 0.0)) continue;
    const double p = x / T;
    ent -= p * log(p);
    if (val) {
      const double v = val[i];
      mean += p * v;
      if (dir) {
        const double ch = q.is_percent ? v : v - vo;
        if (ch > 0.0) up += x; else if (ch < 0.0) dn += x; else fl += x;
      }
    }
  }
  ent = stats_sum(ent, sh, par);
  mean = stats_sum(mean, sh, par);
  dn = stats_sum(dn, sh, par);
  fl = stats_sum(fl, sh, par);
  up = stats_sum(up, sh, par);
  double var = 0.0;
  if (val)
    for (int i = i0; i < i1; ++i) {
      const double x = at(i);
      if (!(x > 0.0)) continue;
      const double dv = val[i] - mean;
      var += (x / T) * (dv * dv);
    }
  var = stats_sum(var, sh, par);
  if (tid == 0) {
    st[0] = T;
    st[1] = ent;
    st[2] = val ? mean : nan;
    st[3] = val ? var : nan;
    st[4] = dir ? dn / T : nan;
    st[5] = dir ? fl / T : nan;
    st[6] = dir ? up / T : nan;
    st[7] = (double)fmaxf(fmaxf(sh.f[0], sh.f[1]), fmaxf(sh.f[2], sh.f[3])) / T;
  }
  // quantiles: the first token with mass whose inclusive prefix (the tree's) reaches level * T; should rounding
  // leave none, the last token with mass
  for (int k = 0; k < nq; ++k) {
    const double target = batch.level[k] * T;
    int hit = V;
    double p = ex;
    for (int i = i0; i < i1; ++i) {
      const double x = at(i);
      p += x;
      if (x > 0.0 && p >= target) { hit = i; break; }
    }
    hit = stats_ext<true>(hit, sh, par);
    if (tid == 0) qt[k] = hit < V ? hit : lastpos;
  }
}

}  // namespace

hipError_t mmt_launch_forecast_law(const ForecastBatch& b, int n, bool onchip, int64_t rows, ForecastRowInfo* info,
                                   hipStream_t s) {
  const dim3 grid((unsigned)rows, (unsigned)n);
  if (onchip)
    hipLaunchKernelGGL(forecast_law_kernel<true>, grid, dim3(SAMPLE_THREADS), 0, s, b, rows, info);
  else
    hipLaunchKernelGGL(forecast_law_kernel<false>, grid, dim3(SAMPLE_THREADS), 0, s, b, rows, info);
  return hipGetLastError();
}

hipError_t mmt_launch_forecast_weights(const ForecastWeights& w, int count, int batch, int samples, int j0, int j1,
                                       const double* logw, double* logw_out, const ForecastRowInfo* info,
                                       float* omega, ForecastPromptInfo* pinfo, hipStream_t s) {
  hipLaunchKernelGGL(forecast_weights_kernel, dim3((unsigned)batch, (unsigned)count), dim3(SAMPLE_THREADS), 0, s, w,
                     batch, samples, j0, j1, logw, logw_out, info, omega, pinfo);
  return hipGetLastError();
}

hipError_t mmt_launch_forecast_mix(const ForecastBatch& b, int n, bool weighted, int batch, int samples,
                                   const ForecastRowInfo* info, const float* omega, const ForecastPromptInfo* pinfo,
                                   hipStream_t s) {
  int vmax = 1;
  for (int k = 0; k < n; ++k) vmax = b.p[k].V > vmax ? b.p[k].V : vmax;
  const int nchunks = (vmax + MIX_COLS - 1) / MIX_COLS;
  const dim3 grid((unsigned)((int64_t)batch * nchunks), (unsigned)n);
  if (weighted)
    hipLaunchKernelGGL(forecast_mix_kernel<true>, grid, dim3(MIX_THREADS), 0, s, b, batch, samples, nchunks, info,
                       omega, pinfo);
  else
    hipLaunchKernelGGL(forecast_mix_kernel<false>, grid, dim3(MIX_THREADS), 0, s, b, batch, samples, nchunks, info,
                       omega, pinfo);
  return hipGetLastError();
}

hipError_t mmt_launch_pmf_stats(const PmfStatsBatch& b, int n, int rows, hipStream_t s) {
  hipLaunchKernelGGL(pmf_stats_kernel, dim3((unsigned)rows, (unsigned)n), dim3(SAMPLE_THREADS), 0, s, b);
  return hipGetLastError();
}

namespace {

// the scratch: [count][rows] row laws, [count][rows] weights, [count][batch] prompt records
struct ScratchPlan { int64_t omega, pinfo, bytes; };
bool scratch_plan(int32_t count, int32_t batch, int32_t samples, ScratchPlan& sp) {
  if (count < 0 || batch < 0 || samples < 1 || (int64_t)batch * samples > 0x7fffffff) return false;
  const int64_t rows = (int64_t)batch * samples;
  if (count > 0 && rows > (int64_t)0x7fffffffffffll / count) return false;
  sp.omega = (int64_t)count * rows * (int64_t)sizeof(ForecastRowInfo);
  sp.pinfo = sp.omega + (((int64_t)count * rows * 4 + 15) & ~(int64_t)15);
  sp.bytes = sp.pinfo + (int64_t)count * batch * (int64_t)sizeof(ForecastPromptInfo);
  return true;
}

}  // namespace

extern "C" {

int64_t mmt_forecast_scratch_bytes(int32_t count, int32_t batch, int32_t samples) {
  ScratchPlan sp;
  return scratch_plan(count, batch, samples, sp) ? sp.bytes : -1;
}

int mmt_forecast_multi(void* stream, int32_t count, int32_t batch, int32_t samples, const int32_t* V,
                       const float* const* logits, const int64_t* row_stride, const float* temperature,
                       const int32_t* top_k, const float* top_p, float* const* pmf, const int64_t* pmf_stride,
                       int32_t wcount, const float* const* logprob, const int64_t* lp_stride, int32_t j0, int32_t j1,
                       const double* logw, double* logw_out, double* const* ess, int32_t* const* live,
                       void* scratch, int64_t scratch_bytes) {
  if (count < 0 || batch < 0 || samples < 1) return MMT_ERR_INVALID;
  if ((int64_t)batch * samples > 0x7fffffff) return MMT_ERR_INVALID;
  if (wcount < 0 || wcount > MMT_MAX_GROUP || j0 < 0 || j1 < j0) return MMT_ERR_INVALID;
  if (count == 0) return MMT_OK;
  if (!V || !logits || !row_stride || !temperature || !top_k || !top_p || !pmf || !pmf_stride)
    return MMT_ERR_INVALID;
  for (int p = 0; p < count; ++p) {  // every problem before any launch, by mmt_sample's own rules
    if (V[p] < 1 || row_stride[p] < V[p] || !(temperature[p] >= 0.0f) || top_k[p] < 0 || top_p[p] != top_p[p] ||
        pmf_stride[p] < V[p])
      return MMT_ERR_INVALID;
    if (batch > 0 && (!logits[p] || !pmf[p])) return MMT_ERR_INVALID;
    if (V[p] > SAMPLE_MAX_V) return MMT_ERR_UNSUPPORTED;
  }
  const bool weighted = wcount > 0 || logw != nullptr;
  if (logw_out && (!weighted || logw_out == logw)) return MMT_ERR_INVALID;
  ForecastWeights fw{};
  fw.count = j1 > j0 ? wcount : 0;
  if (fw.count > 0 && (!logprob || !lp_stride)) return MMT_ERR_INVALID;
  for (int g = 0; g < fw.count; ++g) {
    if (batch > 0 && !logprob[g]) return MMT_ERR_INVALID;
    if (lp_stride[g] < j1) return MMT_ERR_INVALID;
    fw.lp[g] = logprob[g];
    fw.stride[g] = lp_stride[g];
  }
  ScratchPlan sp;
  if (!scratch_plan(count, batch, samples, sp)) return MMT_ERR_INVALID;
  if (batch > 0 && (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < sp.bytes)) return MMT_ERR_INVALID;
  if (weighted && samples > FC_MAX_S) return MMT_ERR_UNSUPPORTED;
  if (weighted && count > 65535) return MMT_ERR_UNSUPPORTED;
  int vmax = 1;
  for (int p = 0; p < count; ++p) vmax = V[p] > vmax ? V[p] : vmax;
  if ((int64_t)batch * ((vmax + MIX_COLS - 1) / MIX_COLS) > 0x7fffffff) return MMT_ERR_UNSUPPORTED;
  if (batch == 0) return MMT_OK;

  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)batch * samples;
  ForecastRowInfo* info = reinterpret_cast<ForecastRowInfo*>(scratch);
  float* omega = reinterpret_cast<float*>(static_cast<char*>(scratch) + sp.omega);
  ForecastPromptInfo* pinfo = reinterpret_cast<ForecastPromptInfo*>(static_cast<char*>(scratch) + sp.pinfo);
  auto fill = [&](ForecastProblem& q, int p) {
    const int greedy = temperature[p] == 0.0f ? 1 : 0;
    q.logits = logits[p];
    q.row_stride = row_stride[p];
    q.pmf = pmf[p];
    q.pmf_stride = pmf_stride[p];
    q.ess = ess ? ess[p] : nullptr;
    q.live = live ? live[p] : nullptr;
    q.inv_t = greedy ? 1.0f : 1.0f / temperature[p];
    q.top_p = top_p[p];
    q.V = V[p];
    q.greedy = greedy;
    q.top_k = top_k[p];
    q.index = p;
  };
  // the row laws: the rows that fit LDS first, then the re-read ones, each in chunks of MMT_MAX_GROUP problems
  for (int large = 0; large < 2; ++large) {
    ForecastBatch fb;
    int n = 0;
    for (int p = 0; p <= count; ++p) {
      if (p < count && (V[p] > SAMPLE_ONCHIP) == (large != 0)) fill(fb.p[n++], p);
      if (n == MMT_MAX_GROUP || (p == count && n > 0)) {
        for (int k = n; k < MMT_MAX_GROUP; ++k) fb.p[k] = fb.p[0];  // never read: grid.y == n
        if (mmt_launch_forecast_law(fb, n, !large, rows, info, s) != hipSuccess) return MMT_ERR_HIP;
        n = 0;
      }
    }
  }
  if (weighted &&
      mmt_launch_forecast_weights(fw, count, batch, samples, j0, j1, logw, logw_out, info, omega, pinfo, s) != hipSuccess)
    return MMT_ERR_HIP;
  for (int p0 = 0; p0 < count; p0 += MMT_MAX_GROUP) {
    ForecastBatch fb;
    const int n = count - p0 < MMT_MAX_GROUP ? count - p0 : MMT_MAX_GROUP;
    for (int k = 0; k < MMT_MAX_GROUP; ++k) fill(fb.p[k], p0 + (k < n ? k : 0));
    if (mmt_launch_forecast_mix(fb, n, weighted, batch, samples, info, omega, pinfo, s) != hipSuccess)
      return MMT_ERR_HIP;
  }
  return MMT_OK;
}

int mmt_pmf_stats(void* stream, int32_t count, int32_t rows, const int32_t* V, const float* const* pmf,
                  const int64_t* pmf_stride, const double* const* values, const int32_t* is_percent,
                  const int64_t* const* origin, const int64_t* origin_stride, int32_t nq, const double* levels,
                  double* const* stats, int32_t* const* qtok) {
  if (count < 0 || rows < 0 || nq < 0 || nq > MMT_PMF_MAX_Q) return MMT_ERR_INVALID;
  if (nq > 0 && !levels) return MMT_ERR_INVALID;
  for (int k = 0; k < nq; ++k)
    if (!(levels[k] > 0.0 && levels[k] < 1.0)) return MMT_ERR_INVALID;
  if (count == 0) return MMT_OK;
  if (!V || !pmf || !pmf_stride || !stats || (nq > 0 && !qtok) || (origin && !origin_stride)) return MMT_ERR_INVALID;
  for (int p = 0; p < count; ++p) {
    if (V[p] < 1 || pmf_stride[p] < V[p]) return MMT_ERR_INVALID;
    if (rows > 0 && (!pmf[p] || !stats[p] || (nq > 0 && !qtok[p]))) return MMT_ERR_INVALID;
    if (V[p] > SAMPLE_MAX_V) return MMT_ERR_UNSUPPORTED;
  }
  if (rows == 0) return MMT_OK;
  for (int p0 = 0; p0 < count; p0 += MMT_MAX_GROUP) {
    PmfStatsBatch sb;
    const int n = count - p0 < MMT_MAX_GROUP ? count - p0 : MMT_MAX_GROUP;
    for (int k = 0; k < MMT_MAX_GROUP; ++k) {
      const int p = p0 + (k < n ? k : 0);
      PmfStatsProblem& q = sb.p[k];
      q.pmf = pmf[p];
      q.stride = pmf_stride[p];
      q.values = values ? values[p] : nullptr;
      q.origin = origin ? origin[p] : nullptr;
      q.origin_stride = origin ? origin_stride[p] : 0;
      q.stats = stats[p];
      q.qtok = qtok ? qtok[p] : nullptr;
      q.V = V[p];
      q.is_percent = is_percent ? is_percent[p] : 0;
    }
    for (int k = 0; k < MMT_PMF_MAX_Q; ++k) sb.level[k] = k < nq ? levels[k] : 0.5;
    sb.nq = nq;
    if (mmt_launch_pmf_stats(sb, n, rows, (hipStream_t)stream) != hipSuccess) return MMT_ERR_HIP;
  }
  return MMT_OK;
}

}  // extern "C"
