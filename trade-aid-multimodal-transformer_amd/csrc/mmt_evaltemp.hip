// Temperature sweep of the evaluation logits (mmt.h: mmt_eval_temperatures): per row (b, t) and temperature k one
// record of four fp64 fields (log score of yb, the three direction masses) under the law mmt_sample draws from at
// that temperature, then the tables a fit of the temperature needs: per k the summed log score and the reliability
// cells.
//
// Three launches a chunk of up to 8 problems (one more when some V > 8192):
//   record    grid (batch x (T - t_begin), problems), 256 threads, a row per workgroup. The RAW row goes into LDS
//             once (row_max at inv_t 1, NaN as -inf) with the direction class of every token beside it; since
//             inv_t > 0 and rounding is monotone the maximum of the scaled row is the scaled maximum, so the one
//             block_max serves all K. Then, ET_GROUP temperatures at a time, one walk of the thread's chunk
//             [t c, t c + c) of row_sums: z = raw * inv_t (the sampler's one fp32 multiply), e = weight(z, m), added
//             to S and to the mass of its class; the 4 x ET_GROUP sums go through row_sums' tree (serial per thread,
//             shift scan over the lanes, wave totals left to right) behind one barrier, and thread j of the group
//             writes the record of its temperature.
//   position  grid (T - t_begin, K, problems), 256 threads: the records of the position's rows at one temperature
//             pass through LDS in tiles of 128 rows, each with its realised sign; thread j owns cells j, j + 256,
//             j + 512 of the partial table (2 sums, 9 x bins reliability cells; at most 578) and adds what row b
//             gives its cells, b ascending. The partials go to the scratch.
//   finalize  grid (ceil(K cells / 256), problems): a cell is the sum over t ascending of the positions' partials,
//             written or added to what the buffer holds.
// No float atomics and no data-dependent order, so a launch is bit-identical run to run, and a problem's bits do
// not depend on its company: a workgroup reads its own problem and nothing else.
#include <cmath>

#include "mmt.h"
#include "mmt_common.h"
#include "mmt_eval_dev.h"
#include "mmt_kernels.h"
#include "mmt_sample_dev.h"

namespace {

constexpr int ET_REC = 4;
constexpr int ET_GROUP = 4;      // temperatures behind one barrier
constexpr int ET_TILE = 128;     // rows of one position held in LDS at a time
constexpr int ET_ROW = ET_REC + 1;  // a tile row: the record and the realised sign
constexpr int ET_THREADS = 256;  // position / finalize workgroup
constexpr int ET_MAX_BINS = 64;
constexpr int ET_OWN = (2 + 9 * ET_MAX_BINS + ET_THREADS - 1) / ET_THREADS;  // cells a thread owns at most

struct EvalTempShared { double d[2][ET_GROUP][4][SAMPLE_WAVES]; };

// the sampler's step 1 on a logit already freed of NaN: one fp32 multiply, never fused into what follows
__device__ __forceinline__ float et_scale(float x, float inv_t) {
  const float z = __fmul_rn(x, inv_t);
  return z != z ? -INFINITY : z;
}

template <bool ONCHIP>
__global__ __launch_bounds__(SAMPLE_THREADS) void evaltemp_record_kernel(EvalTempBatch batch, int T, int t_begin) {
  __shared__ float zs[ONCHIP ? SAMPLE_ONCHIP : 1];
  __shared__ signed char cls[ONCHIP ? SAMPLE_ONCHIP : 1];
  __shared__ SampleShared sh;
  __shared__ EvalTempShared es;
  const EvalTempProblem& q = batch.p[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = q.V, K = batch.K;
  const int nt = T - t_begin;
  const int64_t r = (int64_t)(blockIdx.x / nt) * T + t_begin + blockIdx.x % nt;
  const float* row = q.logits + r * V;
  double* out = q.rec + r * K * ET_REC;
  int par = 0;
  auto raw = [&](int i) -> float { return ONCHIP ? zs[i] : scaled_logit(row, i, 1.0f); };
  const float M = row_max<ONCHIP>(zs, row, V, 1.0f, sh, par);
  const int64_t x = q.xb[r], y = q.yb[r];
  // a dead row, for every temperature alike. Uniform: every thread holds M, x, y.
  if (M == -INFINITY || x < 0 || x >= V || y < 0 || y >= V) {
    for (int i = tid; i < K * ET_REC; i += SAMPLE_THREADS) out[i] = ev_nan();
    return;
  }
  const double* val = q.values;
  const int pct = q.is_percent;
  const double vo = (val && !pct) ? val[x] : 0.0;
  if (ONCHIP && val) {
    for (int i = tid; i < V; i += SAMPLE_THREADS) cls[i] = (signed char)ev_sign(val[i], vo, pct);
    __syncthreads();  // the walk below reads chunks, not strides
  }
  auto sgn = [&](int i) -> int { return ONCHIP ? (int)cls[i] : ev_sign(val[i], vo, pct); };
  // the thread's chunk: row_sums' assignment
  const int c = ((V + SAMPLE_THREADS - 1) / SAMPLE_THREADS) | 1;
  const int64_t i0l = (int64_t)tid * c;
  const int i0 = i0l < V ? (int)i0l : V, i1 = i0l + c < V ? (int)(i0l + c) : V;
  const float xy = raw((int)y);
  int ep = 0;
  for (int k0 = 0; k0 < K; k0 += ET_GROUP) {
    float inv[ET_GROUP], m[ET_GROUP];
    double v[ET_GROUP][4];  // S, down, flat, up
#pragma unroll
    for (int j = 0; j < ET_GROUP; ++j) {
      inv[j] = batch.inv_t[k0 + j < K ? k0 + j : K - 1];  // past K: the last one again, never written
      m[j] = et_scale(M, inv[j]);
      v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0.0;
    }
    for (int i = i0; i < i1; ++i) {
      const float xi = raw(i);
      const int sg = val ? sgn(i) : 0;
#pragma unroll
      for (int j = 0; j < ET_GROUP; ++j) {
        const double e = (double)weight(et_scale(xi, inv[j]), m[j]);
        v[j][0] += e;
        if (val) {  // a leaf outside a class adds 0 to it, which changes nothing
          v[j][1] += sg < 0 ? e : 0.0;
          v[j][2] += sg == 0 ? e : 0.0;
          v[j][3] += sg > 0 ? e : 0.0;
        }
      }
    }
    // row_sums' tree for all sums at once: shift scan over the lanes, lane 63 holds the wave total
    const int nf = val ? 4 : 1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
      for (int j = 0; j < ET_GROUP; ++j) {
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          if (f < nf) {
            const double n = __shfl_up(v[j][f], o, 64);
            if (lane >= o) v[j][f] += n;
          }
        }
      }
    }
    if (lane == 63) {
#pragma unroll
      for (int j = 0; j < ET_GROUP; ++j) {
#pragma unroll
        for (int f = 0; f < 4; ++f) es.d[ep][j][f][wave] = v[j][f];
      }
    }
    __syncthreads();  // es is double buffered: a slot is rewritten two groups later, after a barrier every reader passed
    if (tid < ET_GROUP && k0 + tid < K) {
      const double(&d)[4][SAMPLE_WAVES] = es.d[ep][tid];
      const float it = batch.inv_t[k0 + tid];
      const float mk = et_scale(M, it), zy = et_scale(xy, it);
      const double S = ((d[0][0] + d[0][1]) + d[0][2]) + d[0][3];
      double* o = out + (k0 + tid) * ET_REC;
      o[0] = (double)(zy == -INFINITY ? -INFINITY : token_logprob(zy, mk, S));
#pragma unroll
      for (int f = 1; f < 4; ++f) o[f] = val ? (((d[f][0] + d[f][1]) + d[f][2]) + d[f][3]) / S : ev_nan();
    }
    ep ^= 1;
  }
}

// what one tile row (the record and the realised sign) gives one cell of its position's partial table
__device__ __forceinline__ double et_contrib(int cell, const double* __restrict__ r, int bins) {
  if (r[0] != r[0]) return 0.0;  // a dead row
  if (cell == 0) return 1.0;
  if (cell == 1) return -r[0];
  if (r[1] != r[1]) return 0.0;  // no direction
  const int c = cell - 2;
  const int d = c / (3 * bins), bin = (c / 3) % bins, f = c % 3;
  const double p = r[1 + d];
  if (ev_bin(p, bins) != bin) return 0.0;
  return f == 0 ? 1.0 : (f == 1 ? p : (r[ET_REC] == (double)(d - 1) ? 1.0 : 0.0));
}

__global__ __launch_bounds__(ET_THREADS) void evaltemp_position_kernel(EvalTempBatch batch, int nb, int T, int t_begin,
                                                                       int bins) {
  __shared__ double tile[ET_TILE * ET_ROW];
  const EvalTempProblem& q = batch.p[blockIdx.z];
  const int tid = threadIdx.x, t = t_begin + blockIdx.x, k = blockIdx.y, K = batch.K;
  const int ncell = 2 + 9 * bins;
  const double* val = q.values;
  const int pct = q.is_percent;
  double acc[ET_OWN];
#pragma unroll
  for (int j = 0; j < ET_OWN; ++j) acc[j] = 0.0;
  for (int b0 = 0; b0 < nb; b0 += ET_TILE) {
    const int n = nb - b0 < ET_TILE ? nb - b0 : ET_TILE;
    __syncthreads();  // the previous tile has been read
    for (int j = tid; j < n; j += ET_THREADS) {
      const int64_t r = (int64_t)(b0 + j) * T + t;
      const double* rc = q.rec + (r * K + k) * ET_REC;
      double* dst = tile + j * ET_ROW;
#pragma unroll
      for (int f = 0; f < ET_REC; ++f) dst[f] = rc[f];
      // a row with a direction is live and has values: xb and yb are inside the vocabulary
      dst[ET_REC] = rc[1] == rc[1] ? (double)ev_sign(val[q.yb[r]], pct ? 0.0 : val[q.xb[r]], pct) : ev_nan();
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
#pragma unroll
      for (int o = 0; o < ET_OWN; ++o) {
        const int cell = tid + o * ET_THREADS;
        if (cell < ncell) acc[o] += et_contrib(cell, tile + j * ET_ROW, bins);
      }
    }
  }
  double* part = q.part + ((int64_t)t * K + k) * ncell;
#pragma unroll
  for (int o = 0; o < ET_OWN; ++o) {
    const int cell = tid + o * ET_THREADS;
    if (cell < ncell) part[cell] = acc[o];
  }
}

__global__ __launch_bounds__(ET_THREADS) void evaltemp_finalize_kernel(EvalTempBatch batch, int T, int t_begin,
                                                                       int bins, int accumulate) {
  const EvalTempProblem& q = batch.p[blockIdx.y];
  const int ncell = 2 + 9 * bins, all = batch.K * ncell;
  const int g = blockIdx.x * ET_THREADS + threadIdx.x;
  if (g >= all) return;
  double acc = 0.0;
  for (int t = t_begin; t < T; ++t) acc += q.part[(int64_t)t * all + g];
  const int k = g / ncell, cell = g % ncell;
  double* dst = cell < 2 ? q.sum + k * 2 + cell : q.rel + (int64_t)k * 9 * bins + (cell - 2);
  *dst = accumulate ? *dst + acc : acc;
}

// the scratch: [count][batch, T, K, 4] records (used where the caller keeps none), [count][T][K][2 + 9 bins] partials
struct ScratchPlan { int64_t rec_each, part, part_each, bytes; };
bool scratch_plan(int32_t count, int32_t batch, int32_t T, int32_t bins, int32_t K, ScratchPlan& sp) {
  if (count < 0 || batch < 0 || T < 0 || bins < 1 || bins > ET_MAX_BINS || K < 1 || K > MMT_ET_MAX_K) return false;
  if ((int64_t)batch * T > 0x7fffffff) return false;
  sp.rec_each = (int64_t)batch * T * K * ET_REC * (int64_t)sizeof(double);
  sp.part_each = (int64_t)T * K * (2 + 9 * bins) * (int64_t)sizeof(double);
  if (count > 0 && sp.rec_each + sp.part_each > (int64_t)0x3fffffffffffffffll / count) return false;
  sp.part = (int64_t)count * sp.rec_each;
  sp.bytes = sp.part + (int64_t)count * sp.part_each;
  return true;
}

}  // namespace

hipError_t mmt_launch_evaltemp_records(const EvalTempBatch& b, int n, bool onchip, int batch, int T, int t_begin,
                                       hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)batch * (T - t_begin)), (unsigned)n);
  if (onchip)
    hipLaunchKernelGGL(evaltemp_record_kernel<true>, grid, dim3(SAMPLE_THREADS), 0, s, b, T, t_begin);
  else
    hipLaunchKernelGGL(evaltemp_record_kernel<false>, grid, dim3(SAMPLE_THREADS), 0, s, b, T, t_begin);
  return hipGetLastError();
}

hipError_t mmt_launch_evaltemp_tables(const EvalTempBatch& b, int n, int batch, int T, int t_begin, int bins,
                                      int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(evaltemp_position_kernel, dim3((unsigned)(T - t_begin), (unsigned)b.K, (unsigned)n),
                     dim3(ET_THREADS), 0, s, b, batch, T, t_begin, bins);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int all = b.K * (2 + 9 * bins);
  hipLaunchKernelGGL(evaltemp_finalize_kernel, dim3((unsigned)((all + ET_THREADS - 1) / ET_THREADS), (unsigned)n),
                     dim3(ET_THREADS), 0, s, b, T, t_begin, bins, accumulate);
  return hipGetLastError();
}

extern "C" {

int64_t mmt_eval_temperatures_scratch_bytes(int32_t count, int32_t batch, int32_t T, int32_t bins, int32_t K) {
  ScratchPlan sp;
  return scratch_plan(count, batch, T, bins, K, sp) ? sp.bytes : -1;
}

int mmt_eval_temperatures(void* stream, int32_t count, int32_t batch, int32_t T, int32_t t_begin, int32_t bins,
                          int32_t accumulate, int32_t K, const float* temperatures, const int32_t* V,
                          const float* const* logits, const int64_t* const* xb, const int64_t* const* yb,
                          const double* const* values, const int32_t* is_percent, double* const* rec,
                          double* const* sum, double* const* rel, void* scratch, int64_t scratch_bytes) {
  ScratchPlan sp;
  if (!scratch_plan(count, batch, T, bins, K, sp)) return MMT_ERR_INVALID;
  if (t_begin < 0 || t_begin > T || !temperatures) return MMT_ERR_INVALID;
  for (int k = 0; k < K; ++k) {
    const float tau = temperatures[k];
    if (!std::isfinite(tau) || !(tau > 0.0f) || (k > 0 && !(tau > temperatures[k - 1]))) return MMT_ERR_INVALID;
  }
  if (count == 0) return MMT_OK;
  if (!V || !logits || !xb || !yb || !sum || !rel) return MMT_ERR_INVALID;
  const bool work = batch > 0 && t_begin < T;
  for (int p = 0; p < count; ++p) {  // every problem before any launch
    if (V[p] < 1) return MMT_ERR_INVALID;
    if (work && (!logits[p] || !xb[p] || !yb[p] || !sum[p] || !rel[p])) return MMT_ERR_INVALID;
    if (V[p] > SAMPLE_MAX_V) return MMT_ERR_UNSUPPORTED;
  }
  if (batch > 0 && (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < sp.bytes)) return MMT_ERR_INVALID;
  if (!work) return MMT_OK;

  hipStream_t s = (hipStream_t)stream;
  char* sc = static_cast<char*>(scratch);
  for (int p0 = 0; p0 < count; p0 += MMT_MAX_GROUP) {
    const int n = count - p0 < MMT_MAX_GROUP ? count - p0 : MMT_MAX_GROUP;
    EvalTempBatch all;
    all.K = K;
    for (int k = 0; k < MMT_ET_MAX_K; ++k) all.inv_t[k] = 1.0f / temperatures[k < K ? k : K - 1];
    for (int k = 0; k < MMT_MAX_GROUP; ++k) {  // entries past n repeat the first and are never read
      const int p = p0 + (k < n ? k : 0);
      EvalTempProblem& q = all.p[k];
      q.logits = logits[p];
      q.xb = xb[p];
      q.yb = yb[p];
      q.values = values ? values[p] : nullptr;
      q.rec = rec && rec[p] ? rec[p] : reinterpret_cast<double*>(sc + (int64_t)p * sp.rec_each);
      q.sum = sum[p];
      q.rel = rel[p];
      q.part = reinterpret_cast<double*>(sc + sp.part + (int64_t)p * sp.part_each);
      q.V = V[p];
      q.is_percent = is_percent ? is_percent[p] : 0;
    }
    // the records: the rows that fit LDS, then the re-read ones (a second launch, only when there are any)
    for (int large = 0; large < 2; ++large) {
      EvalTempBatch eb = all;
      int m = 0;
      for (int k = 0; k < n; ++k)
        if ((all.p[k].V > SAMPLE_ONCHIP) == (large != 0)) eb.p[m++] = all.p[k];
      if (m == 0) continue;
      for (int k = m; k < MMT_MAX_GROUP; ++k) eb.p[k] = eb.p[0];
      if (mmt_launch_evaltemp_records(eb, m, !large, batch, T, t_begin, s) != hipSuccess) return MMT_ERR_HIP;
    }
    if (mmt_launch_evaltemp_tables(all, n, batch, T, t_begin, bins, accumulate, s) != hipSuccess) return MMT_ERR_HIP;
  }
  return MMT_OK;
}

}  // extern "C"
