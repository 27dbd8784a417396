// Evaluation at every position (mmt.h: mmt_eval_positions): per row (b, t) of the evaluation forward's logits one
// record of eight fp64 fields (log score, direction masses, mid-PIT, rank, predicted and realised sign), then the
// tables: per position, per reliability bin, per PIT bin.
//
// Three launches a chunk of up to 8 problems (one more when some V > 8192):
//   record    grid (batch x (T - t_begin), problems), 256 threads, a row per workgroup: the sampler's own front
//             (row_max, row_sums of mmt_sample_dev.h, so m and S are the sampler's and the log score is bit for bit
//             mmt_score_multi's), then one walk of the thread's chunk [t c, t c + c) for the four masses (down, flat,
//             up, below yb), the rank count and the first maximum; the masses go through the same tree as S (serial
//             per thread, shift scan over the lanes, wave totals left to right), all four behind one barrier.
//   position  grid (T, problems), 256 threads, a position per workgroup: the records of the position's rows pass
//             through LDS in tiles of 128 rows; thread j owns cells j, j + 256, j + 512 of the position's partial
//             table (8 position fields, 9 x bins reliability cells, bins PIT cells; at most 648) and adds what row
//             b gives its cells, b ascending. The position fields go to pos (one add with `accumulate`), the rest to
//             the scratch.
//   finalize  grid (problems), 256 threads: a reliability / PIT cell is the sum over t ascending of the positions'
//             partials, written or added to what the buffer holds.
// No float atomics and no data-dependent order, so a launch is bit-identical run to run, and a problem's bits do
// not depend on its company: a workgroup reads its own problem and nothing else.
#include "mmt.h"
#include "mmt_common.h"
#include "mmt_eval_dev.h"
#include "mmt_kernels.h"
#include "mmt_sample_dev.h"

namespace {

constexpr int EV_REC = 8;
constexpr int EV_TILE = 128;     // rows of one position held in LDS at a time
constexpr int EV_THREADS = 256;  // position / finalize workgroup
constexpr int EV_MAX_BINS = 64;
constexpr int EV_OWN = (8 + 10 * EV_MAX_BINS + EV_THREADS - 1) / EV_THREADS;  // cells a thread owns at most

struct EvalShared {
  double d[4][SAMPLE_WAVES];
  int cnt[SAMPLE_WAVES];
  int first[SAMPLE_WAVES];
};

template <bool ONCHIP>
__global__ __launch_bounds__(SAMPLE_THREADS) void evalpos_record_kernel(EvalPosBatch batch, int T, int t_begin) {
  __shared__ float zs[ONCHIP ? SAMPLE_ONCHIP : 1];
  __shared__ SampleShared sh;
  __shared__ EvalShared es;
  const EvalPosProblem& q = batch.p[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = q.V;
  const int nt = T - t_begin;
  const int64_t r = (int64_t)(blockIdx.x / nt) * T + t_begin + blockIdx.x % nt;
  const float* row = q.logits + r * V;
  double* out = q.rec + r * EV_REC;
  int par = 0;
  auto zat = [&](int i) -> float { return ONCHIP ? zs[i] : scaled_logit(row, i, 1.0f); };
  const float m = row_max<ONCHIP>(zs, row, V, 1.0f, sh, par);
  const int64_t x = q.xb[r], y = q.yb[r];
  // a dead row: no finite logit, or a token outside the vocabulary (never read). Uniform: every thread holds m, x, y.
  if (m == -INFINITY || x < 0 || x >= V || y < 0 || y >= V) {
    if (tid < EV_REC) out[tid] = ev_nan();
    return;
  }
  const RowSums rs = row_sums(zat, V, m, 0u, sh, par);
  const float zy = zat((int)y);
  const double* val = q.values;
  const int pct = q.is_percent;
  const double vo = (val && !pct) ? val[x] : 0.0;

  double v[4] = {0.0, 0.0, 0.0, 0.0};  // down, flat, up, below yb
  int cnt = 0, first = V;
  for (int i = rs.i0; i < rs.i1; ++i) {
    const float z = zat(i);
    const double e = (double)weight(z, m);
    if (val) {  // a leaf outside a class adds 0 to it, which changes nothing
      const int sg = ev_sign(val[i], vo, pct);
      v[0] += sg < 0 ? e : 0.0;
      v[1] += sg == 0 ? e : 0.0;
      v[2] += sg > 0 ? e : 0.0;
    }
    v[3] += i < y ? e : 0.0;
    cnt += z > zy ? 1 : 0;
    if (z == m && first == V) first = i;
  }
  // row_sums' tree for the four masses at once: shift scan over the lanes, lane 63 holds the wave total
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double n = __shfl_up(v[k], o, 64);
      if (lane >= o) v[k] += n;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    first = min(first, __shfl_xor(first, o, 64));
  }
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < 4; ++k) es.d[k][wave] = v[k];
    es.cnt[wave] = cnt;
    es.first[wave] = first;
  }
  __syncthreads();
  if (tid != 0) return;
  double tot[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) tot[k] = ((es.d[k][0] + es.d[k][1]) + es.d[k][2]) + es.d[k][3];
  cnt = es.cnt[0] + es.cnt[1] + es.cnt[2] + es.cnt[3];
  first = min(min(es.first[0], es.first[1]), min(es.first[2], es.first[3]));
  const double S = rs.S;
  out[0] = (double)(zy == -INFINITY ? -INFINITY : token_logprob(zy, m, S));
  out[1] = val ? tot[0] / S : ev_nan();
  out[2] = val ? tot[1] / S : ev_nan();
  out[3] = val ? tot[2] / S : ev_nan();
  out[4] = (tot[3] + 0.5 * (double)weight(zy, m)) / S;
  out[5] = (double)cnt;
  out[6] = val ? (double)ev_sign(val[first], vo, pct) : ev_nan();
  out[7] = val ? (double)ev_sign(val[y], vo, pct) : ev_nan();
}

// what one record gives one cell of its position's partial table; 0 where it gives nothing
__device__ __forceinline__ double ev_contrib(int cell, const double* __restrict__ r, int bins) {
  if (r[5] != r[5]) return 0.0;  // a dead row
  const bool dir = r[6] == r[6];
  if (cell < 8) {
    switch (cell) {
      case 0: return 1.0;
      case 1: return dir && r[6] == r[7] ? 1.0 : 0.0;
      case 2: return dir && r[6] != r[7] ? 1.0 : 0.0;
      case 3: return dir ? (r[6] < 0.0 ? r[1] : (r[6] > 0.0 ? r[3] : r[2])) : 0.0;
      case 4: return -r[0];
      case 5: return r[5] == 0.0 ? 1.0 : 0.0;
      case 6: return dir ? 1.0 : 0.0;
      default: return dir ? (r[7] < 0.0 ? r[1] : (r[7] > 0.0 ? r[3] : r[2])) : 0.0;
    }
  }
  const int c = cell - 8;
  if (c < 9 * bins) {
    if (!dir) return 0.0;
    const int d = c / (3 * bins), bin = (c / 3) % bins, f = c % 3;
    const double p = r[1 + d];
    if (ev_bin(p, bins) != bin) return 0.0;
    return f == 0 ? 1.0 : (f == 1 ? p : (r[7] == (double)(d - 1) ? 1.0 : 0.0));
  }
  return ev_bin(r[4], bins) == c - 9 * bins ? 1.0 : 0.0;
}

__global__ __launch_bounds__(EV_THREADS) void evalpos_position_kernel(EvalPosBatch batch, int nb, int T, int t_begin,
                                                                      int bins, int accumulate) {
  __shared__ double tile[EV_TILE * EV_REC];
  const EvalPosProblem& q = batch.p[blockIdx.y];
  const int tid = threadIdx.x, t = blockIdx.x;
  double* pos = q.pos + (int64_t)t * 8;
  if (t < t_begin) {  // contributes nothing (uniform branch)
    if (!accumulate && tid < 8) pos[tid] = 0.0;
    return;
  }
  const int pcells = 10 * bins, ncell = 8 + pcells;
  double acc[EV_OWN];
#pragma unroll
  for (int k = 0; k < EV_OWN; ++k) acc[k] = 0.0;
  for (int b0 = 0; b0 < nb; b0 += EV_TILE) {
    const int n = nb - b0 < EV_TILE ? nb - b0 : EV_TILE;
    __syncthreads();  // the previous tile has been read
    for (int i = tid; i < n * EV_REC; i += EV_THREADS)
      tile[i] = q.rec[((int64_t)(b0 + (i >> 3)) * T + t) * EV_REC + (i & 7)];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
#pragma unroll
      for (int k = 0; k < EV_OWN; ++k) {
        const int cell = tid + k * EV_THREADS;
        if (cell < ncell) acc[k] += ev_contrib(cell, tile + j * EV_REC, bins);
      }
    }
  }
  double* part = q.part + (int64_t)t * pcells;
#pragma unroll
  for (int k = 0; k < EV_OWN; ++k) {
    const int cell = tid + k * EV_THREADS;
    if (cell < 8) pos[cell] = accumulate ? pos[cell] + acc[k] : acc[k];
    else if (cell < ncell) part[cell - 8] = acc[k];
  }
}

__global__ __launch_bounds__(EV_THREADS) void evalpos_finalize_kernel(EvalPosBatch batch, int T, int t_begin, int bins,
                                                                      int accumulate) {
  const EvalPosProblem& q = batch.p[blockIdx.x];
  const int pcells = 10 * bins;
  for (int cell = threadIdx.x; cell < pcells; cell += EV_THREADS) {
    double acc = 0.0;
    for (int t = t_begin; t < T; ++t) acc += q.part[(int64_t)t * pcells + cell];
    double* dst = cell < 9 * bins ? q.rel + cell : q.pit + (cell - 9 * bins);
    *dst = accumulate ? *dst + acc : acc;
  }
}

// the scratch: [count][batch, T, 8] records (used where the caller keeps none), [count][T][10 bins] partials
struct ScratchPlan { int64_t rec_each, part, part_each, bytes; };
bool scratch_plan(int32_t count, int32_t batch, int32_t T, int32_t bins, ScratchPlan& sp) {
  if (count < 0 || batch < 0 || T < 0 || bins < 1 || bins > EV_MAX_BINS) return false;
  if ((int64_t)batch * T > 0x7fffffff) return false;
  sp.rec_each = (int64_t)batch * T * EV_REC * (int64_t)sizeof(double);
  sp.part_each = (int64_t)T * 10 * bins * (int64_t)sizeof(double);
  if (count > 0 && sp.rec_each + sp.part_each > (int64_t)0x3fffffffffffffffll / count) return false;
  sp.part = (int64_t)count * sp.rec_each;
  sp.bytes = sp.part + (int64_t)count * sp.part_each;
  return true;
}

}  // namespace

hipError_t mmt_launch_evalpos_records(const EvalPosBatch& b, int n, bool onchip, int batch, int T, int t_begin,
                                      hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)batch * (T - t_begin)), (unsigned)n);
  if (onchip)
    hipLaunchKernelGGL(evalpos_record_kernel<true>, grid, dim3(SAMPLE_THREADS), 0, s, b, T, t_begin);
  else
    hipLaunchKernelGGL(evalpos_record_kernel<false>, grid, dim3(SAMPLE_THREADS), 0, s, b, T, t_begin);
  return hipGetLastError();
}

hipError_t mmt_launch_evalpos_tables(const EvalPosBatch& b, int n, int batch, int T, int t_begin, int bins,
                                     int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(evalpos_position_kernel, dim3((unsigned)T, (unsigned)n), dim3(EV_THREADS), 0, s, b, batch, T,
                     t_begin, bins, accumulate);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(evalpos_finalize_kernel, dim3((unsigned)n), dim3(EV_THREADS), 0, s, b, T, t_begin, bins,
                     accumulate);
  return hipGetLastError();
}

extern "C" {

int64_t mmt_eval_positions_scratch_bytes(int32_t count, int32_t batch, int32_t T, int32_t bins) {
  ScratchPlan sp;
  return scratch_plan(count, batch, T, bins, sp) ? sp.bytes : -1;
}

int mmt_eval_positions(void* stream, int32_t count, int32_t batch, int32_t T, int32_t t_begin, int32_t bins,
                       int32_t accumulate, const int32_t* V, const float* const* logits, const int64_t* const* xb,
                       const int64_t* const* yb, const double* const* values, const int32_t* is_percent,
                       double* const* rec, double* const* pos, double* const* rel, double* const* pit, void* scratch,
                       int64_t scratch_bytes) {
  ScratchPlan sp;
  if (!scratch_plan(count, batch, T, bins, sp)) return MMT_ERR_INVALID;
  if (t_begin < 0 || t_begin > T) return MMT_ERR_INVALID;
  if (count == 0) return MMT_OK;
  if (!V || !logits || !xb || !yb || !pos || !rel || !pit) return MMT_ERR_INVALID;
  const bool work = batch > 0 && t_begin < T;
  for (int p = 0; p < count; ++p) {  // every problem before any launch
    if (V[p] < 1) return MMT_ERR_INVALID;
    if (work && (!logits[p] || !xb[p] || !yb[p] || !pos[p] || !rel[p] || !pit[p])) return MMT_ERR_INVALID;
    if (V[p] > SAMPLE_MAX_V) return MMT_ERR_UNSUPPORTED;
  }
  if (batch > 0 && (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < sp.bytes)) return MMT_ERR_INVALID;
  if (!work) return MMT_OK;

  hipStream_t s = (hipStream_t)stream;
  char* sc = static_cast<char*>(scratch);
  for (int p0 = 0; p0 < count; p0 += MMT_MAX_GROUP) {
    const int n = count - p0 < MMT_MAX_GROUP ? count - p0 : MMT_MAX_GROUP;
    EvalPosBatch all;
    for (int k = 0; k < MMT_MAX_GROUP; ++k) {  // entries past n repeat the first and are never read
      const int p = p0 + (k < n ? k : 0);
      EvalPosProblem& q = all.p[k];
      q.logits = logits[p];
      q.xb = xb[p];
      q.yb = yb[p];
      q.values = values ? values[p] : nullptr;
      q.rec = rec && rec[p] ? rec[p] : reinterpret_cast<double*>(sc + (int64_t)p * sp.rec_each);
      q.pos = pos[p];
      q.rel = rel[p];
      q.pit = pit[p];
      q.part = reinterpret_cast<double*>(sc + sp.part + (int64_t)p * sp.part_each);
      q.V = V[p];
      q.is_percent = is_percent ? is_percent[p] : 0;
    }
    // the records: the rows that fit LDS, then the re-read ones (a second launch, only when there are any)
    for (int large = 0; large < 2; ++large) {
      EvalPosBatch eb;
      int m = 0;
      for (int k = 0; k < n; ++k)
        if ((all.p[k].V > SAMPLE_ONCHIP) == (large != 0)) eb.p[m++] = all.p[k];
      if (m == 0) continue;
      for (int k = m; k < MMT_MAX_GROUP; ++k) eb.p[k] = eb.p[0];
      if (mmt_launch_evalpos_records(eb, m, !large, batch, T, t_begin, s) != hipSuccess) return MMT_ERR_HIP;
    }
    if (mmt_launch_evalpos_tables(all, n, batch, T, t_begin, bins, accumulate, s) != hipSuccess) return MMT_ERR_HIP;
  }
  return MMT_OK;
}

}  // extern "C"
