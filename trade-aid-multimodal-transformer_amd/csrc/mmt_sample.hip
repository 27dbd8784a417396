// Device-side sampling of generate (mmt.h: mmt_sample): temperature, top-k, top-p, a counter-hash uniform draw,
// the token and its log-probability, one 256-thread workgroup per row, one launch for all rows; mmt_sample_multi:
// the same for several problems (the heads of one joint-rollout step) over the same rows, grid (rows, problems).
//
// No float atomics and no data-dependent summation order: every sum below runs over a fixed assignment of
// elements to threads and a fixed tree (per-thread serial sum, xor-butterfly or shift scan inside a wave, the
// four wave totals added left to right), so a launch is bit-identical run to run and a row's result does not
// depend on which other rows share the launch.
//
// A row's scaled logits z stay in LDS for V <= SAMPLE_ONCHIP (32 KiB; C1's heads are 900 / 13 / 144 / 5); larger
// rows re-read the logits from global memory (L2) and redo the one multiply: the same code, another accessor.
//
// Thresholds (top-k: the k-th largest z; top-p: the largest z whose upper set holds top_p * S) are found by a
// bitwise search over the order-preserving 32-bit key of z: 16 rounds, two bits each, of "how many / how much mass
// at key >= candidate" for the three candidates of the round, most significant bits first. Counts are integers, hence exact. A mass is a sum of non-negative
// terms over a fixed tree with some leaves zeroed; round-to-nearest addition is monotone in each operand, so the
// mass is monotone in the candidate and the search is well defined.
//
// The weights exp(z - m) are fp32 (expf); every sum of them (masses, S, the prefix sums) is fp64, so what
// separates the result from the exact rule is the weights' own rounding, not the length of the row. The kernel is
// latency-bound (a few hundred expf and ~40 barriers per row at V = 900), the fp64 adds are not what it waits for.
#include "mmt.h"
#include "mmt_common.h"
#include "mmt_sample_dev.h"

namespace {

constexpr uint32_t SAMPLE_SALT = 0x53414D50u;  // "SAMP"

// One row: row b = blockIdx.x of one problem, the whole rule of mmt.h. Both kernels below are this body and
// nothing else, so a problem of mmt_sample_multi gives the bits mmt_sample gives with the same arguments.
template <bool ONCHIP>
__device__ __forceinline__ void sample_row(
    float* __restrict__ zs, SampleShared& sh, int V, const float* __restrict__ logits, int64_t row_stride,
    float inv_t, int greedy, int top_k, float top_p, uint32_t key, uint32_t row0, uint32_t pos,
    int64_t* __restrict__ tok, int64_t tok_stride, int64_t* __restrict__ tok_compact, float* __restrict__ logprob,
    int64_t lp_stride) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const float* row = logits + (int64_t)b * row_stride;
  int par = 0;

  auto zat = [&](int i) -> float { return ONCHIP ? zs[i] : scaled_logit(row, i, inv_t); };
  // steps 1 - 4 and the sums of step 5: the row's law (mmt_sample_dev.h), shared with mmt_forecast.hip
  const RowLaw law = row_law<ONCHIP>(zat, zs, row, V, inv_t, greedy, top_k, top_p, sh, par);
  const float m = law.m;

  int64_t* tok_out = tok + (int64_t)b * tok_stride;
  if (m == -INFINITY) {  // no finite logit: token 0, log-probability NaN (uniform branch: every thread holds m)
    if (tid == 0) {
      *tok_out = 0;
      if (tok_compact) tok_compact[b] = 0;
      if (logprob) logprob[(int64_t)b * lp_stride] = __uint_as_float(0x7fc00000u);
    }
    return;
  }

  const uint32_t K = law.K;
  const RowSums& rs = law.rs;
  const int i0 = rs.i0, i1 = rs.i1;
  const double tot = rs.tot, base = rs.base, S = rs.S;
  const bool has_max = rs.has_max;

  const uint32_t h = mmt_hash(key, row0 + (uint32_t)b, pos);
  const double u = ((double)(h >> 8) + 0.5) * (1.0 / 16777216.0);
  const double target = u * S;

  // the owner of the token: the first thread whose inclusive prefix reaches the target (greedy: that holds a
  // maximum); should rounding leave none, the last thread with any weight
  const bool hit = greedy ? has_max : (tot > 0.0 && base + tot >= target);
  const unsigned long long hm = __ballot(hit), nm = __ballot(tot > 0.0);
  if (lane == 0) {
    sh.i[par][wave] = hm ? wave * 64 + (__ffsll((long long)hm) - 1) : SAMPLE_THREADS;
    sh.j[par][wave] = nm ? wave * 64 + (63 - __clzll((long long)nm)) : -1;
  }
  __syncthreads();
  int first = SAMPLE_THREADS, last = -1;
#pragma unroll
  for (int w = 0; w < SAMPLE_WAVES; ++w) {
    first = sh.i[par][w] < first ? sh.i[par][w] : first;
    last = sh.j[par][w] > last ? sh.j[par][w] : last;
  }
  const int owner = first < SAMPLE_THREADS ? first : last;
  if (tid != owner) return;

  int t = -1, lastpos = i0;
  double p = base;
  for (int i = i0; i < i1; ++i) {
    const float z = zat(i);
    if (greedy) {
      if (z == m) { t = i; break; }
      continue;
    }
    const float e = okey(z) >= K ? weight(z, m) : 0.f;
    p += (double)e;
    if (e > 0.f) {
      lastpos = i;
      if (p >= target) { t = i; break; }
    }
  }
  if (t < 0) t = lastpos;
  *tok_out = t;
  if (tok_compact) tok_compact[b] = t;
  if (logprob) {
    logprob[(int64_t)b * lp_stride] = token_logprob(zat(t), m, S);
  }
}

template <bool ONCHIP>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(
    int V, const float* __restrict__ logits, int64_t row_stride, float inv_t, int greedy, int top_k, float top_p,
    uint32_t key, uint32_t row0, uint32_t pos, int64_t* __restrict__ tok, int64_t tok_stride,
    int64_t* __restrict__ tok_compact, float* __restrict__ logprob, int64_t lp_stride) {
  __shared__ float zs[ONCHIP ? SAMPLE_ONCHIP : 1];
  __shared__ SampleShared sh;
  sample_row<ONCHIP>(zs, sh, V, logits, row_stride, inv_t, greedy, top_k, top_p, key, row0, pos, tok, tok_stride,
                     tok_compact, logprob, lp_stride);
}

// mmt_sample_multi: grid (rows, problems), workgroup (b, p) is row b of problem p. The problems travel by value
// in the kernel arguments (8 x 80 bytes); a workgroup reads its own through wave-uniform loads.
struct SampleProblem {
  const float* logits;
  int64_t row_stride;
  int64_t* tok;
  int64_t tok_stride;
  int64_t* tok_compact;
  float* logprob;
  int64_t lp_stride;
  float inv_t, top_p;
  int V, greedy, top_k;
  uint32_t key;
};
struct SampleBatch { SampleProblem p[MMT_MAX_GROUP]; };

template <bool ONCHIP>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_multi_kernel(SampleBatch batch, uint32_t row0, uint32_t pos) {
  __shared__ float zs[ONCHIP ? SAMPLE_ONCHIP : 1];
  __shared__ SampleShared sh;
  const SampleProblem& q = batch.p[blockIdx.y];
  sample_row<ONCHIP>(zs, sh, q.V, q.logits, q.row_stride, q.inv_t, q.greedy, q.top_k, q.top_p, q.key, row0, pos, q.tok,
                     q.tok_stride, q.tok_compact, q.logprob, q.lp_stride);
}

// mmt_score_multi: the log-probability of a GIVEN token under the row's raw softmax, i.e. what sample_row writes
// when it draws that token at temperature 1, top_k 0, top_p 1: row_max with inv_t = 1 (an exact multiply), row_sums
// with K = 0, token_logprob. Workgroup (b, p) is row b of problem p; thread 0 writes.
struct ScoreProblem {
  const float* logits;
  int64_t row_stride;
  const int64_t* tok;
  int64_t tok_stride;
  float* logprob;
  int64_t lp_stride;
  int V;
};
struct ScoreBatch { ScoreProblem p[MMT_MAX_GROUP]; };

template <bool ONCHIP>
__global__ __launch_bounds__(SAMPLE_THREADS) void score_multi_kernel(ScoreBatch batch) {
  __shared__ float zs[ONCHIP ? SAMPLE_ONCHIP : 1];
  __shared__ SampleShared sh;
  const ScoreProblem& q = batch.p[blockIdx.y];
  const int b = blockIdx.x, V = q.V;
  const float* row = q.logits + (int64_t)b * q.row_stride;
  int par = 0;
  auto zat = [&](int i) -> float { return ONCHIP ? zs[i] : scaled_logit(row, i, 1.0f); };
  const float m = row_max<ONCHIP>(zs, row, V, 1.0f, sh, par);
  float* out = q.logprob + (int64_t)b * q.lp_stride;
  const float nan = __uint_as_float(0x7fc00000u);
  if (m == -INFINITY) {  // no finite logit (uniform branch)
    if (threadIdx.x == 0) *out = nan;
    return;
  }
  const RowSums rs = row_sums(zat, V, m, 0u, sh, par);
  if (threadIdx.x != 0) return;
  const int64_t t = q.tok[(int64_t)b * q.tok_stride];
  if (t < 0 || t >= V) {  // refused by the Python layer; never read outside the row
    *out = nan;
    return;
  }
  const float zt = zat((int)t);
  *out = zt == -INFINITY ? -INFINITY : token_logprob(zt, m, rs.S);
}

// mmt_sample's refusals for one problem; MMT_OK when it may launch
int sample_check(int32_t batch, int32_t V, const float* logits, int64_t row_stride, float temperature, int32_t top_k,
                 float top_p, const int64_t* tok) {
  if (batch < 0 || V < 1 || row_stride < V || !(temperature >= 0.0f) || top_k < 0 || top_p != top_p)
    return MMT_ERR_INVALID;
  if (batch > 0 && (!logits || !tok)) return MMT_ERR_INVALID;
  if (V > SAMPLE_MAX_V) return MMT_ERR_UNSUPPORTED;
  return MMT_OK;
}

uint32_t sample_key(uint64_t seed) { return mmt_hash((uint32_t)seed, (uint32_t)(seed >> 32), SAMPLE_SALT); }

}  // namespace

extern "C" {

int mmt_sample(void* stream, int32_t batch, int32_t V, const float* logits, int64_t row_stride, float temperature,
               int32_t top_k, float top_p, uint64_t seed, uint32_t row0, uint32_t pos, int64_t* tok,
               int64_t tok_stride, int64_t* tok_compact, float* logprob, int64_t lp_stride) {
  const int rc = sample_check(batch, V, logits, row_stride, temperature, top_k, top_p, tok);
  if (rc != MMT_OK) return rc;
  if (batch == 0) return MMT_OK;
  const int greedy = temperature == 0.0f ? 1 : 0;
  const float inv_t = greedy ? 1.0f : 1.0f / temperature;
  const uint32_t key = sample_key(seed);
  hipStream_t s = (hipStream_t)stream;
  if (V <= SAMPLE_ONCHIP)
    hipLaunchKernelGGL(sample_kernel<true>, dim3((unsigned)batch), dim3(SAMPLE_THREADS), 0, s, V, logits, row_stride,
                       inv_t, greedy, top_k, top_p, key, row0, pos, tok, tok_stride, tok_compact, logprob, lp_stride);
  else
    hipLaunchKernelGGL(sample_kernel<false>, dim3((unsigned)batch), dim3(SAMPLE_THREADS), 0, s, V, logits, row_stride,
                       inv_t, greedy, top_k, top_p, key, row0, pos, tok, tok_stride, tok_compact, logprob, lp_stride);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_ERR_HIP;
}

int mmt_sample_multi(void* stream, int32_t count, int32_t batch, const int32_t* V, const float* const* logits,
                     const int64_t* row_stride, const float* temperature, const int32_t* top_k, const float* top_p,
                     const uint64_t* seed, uint32_t row0, uint32_t pos, int64_t* const* tok, const int64_t* tok_stride,
                     int64_t* const* tok_compact, float* const* logprob, const int64_t* lp_stride) {
  if (count < 0 || batch < 0) return MMT_ERR_INVALID;
  if (count == 0) return MMT_OK;
  if (!V || !logits || !row_stride || !temperature || !top_k || !top_p || !seed || !tok || !tok_stride ||
      (logprob && !lp_stride))
    return MMT_ERR_INVALID;
  for (int p = 0; p < count; ++p) {  // every problem before any launch
    const int rc = sample_check(batch, V[p], logits[p], row_stride[p], temperature[p], top_k[p], top_p[p], tok[p]);
    if (rc != MMT_OK) return rc;
  }
  if (batch == 0) return MMT_OK;
  hipStream_t s = (hipStream_t)stream;
  // the rows that fit LDS first, then the re-read ones (a second launch, only when there are any), each in
  // chunks of MMT_MAX_GROUP problems in the caller's order
  for (int large = 0; large < 2; ++large) {
    SampleBatch sb;
    int n = 0;
    for (int p = 0; p <= count; ++p) {
      if (p < count && (V[p] > SAMPLE_ONCHIP) == (large != 0)) {
        const int greedy = temperature[p] == 0.0f ? 1 : 0;
        SampleProblem& q = sb.p[n++];
        q.logits = logits[p];
        q.row_stride = row_stride[p];
        q.tok = tok[p];
        q.tok_stride = tok_stride[p];
        q.tok_compact = tok_compact ? tok_compact[p] : nullptr;
        q.logprob = logprob ? logprob[p] : nullptr;
        q.lp_stride = logprob ? lp_stride[p] : 0;
        q.inv_t = greedy ? 1.0f : 1.0f / temperature[p];
        q.top_p = top_p[p];
        q.V = V[p];
        q.greedy = greedy;
        q.top_k = top_k[p];
        q.key = sample_key(seed[p]);
      }
      if (n == MMT_MAX_GROUP || (p == count && n > 0)) {
        for (int k = n; k < MMT_MAX_GROUP; ++k) sb.p[k] = sb.p[0];  // never read: grid.y == n
        const dim3 grid((unsigned)batch, (unsigned)n);
        if (large)
          hipLaunchKernelGGL(sample_multi_kernel<false>, grid, dim3(SAMPLE_THREADS), 0, s, sb, row0, pos);
        else
          hipLaunchKernelGGL(sample_multi_kernel<true>, grid, dim3(SAMPLE_THREADS), 0, s, sb, row0, pos);
        if (hipGetLastError() != hipSuccess) return MMT_ERR_HIP;
        n = 0;
      }
    }
  }
  return MMT_OK;
}

int mmt_score_multi(void* stream, int32_t count, int32_t batch, const int32_t* V, const float* const* logits,
                    const int64_t* row_stride, const int64_t* const* tok, const int64_t* tok_stride,
                    float* const* logprob, const int64_t* lp_stride) {
  if (count < 0 || batch < 0) return MMT_ERR_INVALID;
  if (count == 0) return MMT_OK;
  if (!V || !logits || !row_stride || !tok || !tok_stride || !logprob || !lp_stride) return MMT_ERR_INVALID;
  for (int p = 0; p < count; ++p) {  // every problem before any launch
    if (V[p] < 1 || row_stride[p] < V[p]) return MMT_ERR_INVALID;
    if (batch > 0 && (!logits[p] || !tok[p] || !logprob[p])) return MMT_ERR_INVALID;
    if (V[p] > SAMPLE_MAX_V) return MMT_ERR_UNSUPPORTED;
  }
  if (batch == 0) return MMT_OK;
  hipStream_t s = (hipStream_t)stream;
  for (int large = 0; large < 2; ++large) {  // the launch shapes of mmt_sample_multi
    ScoreBatch sb;
    int n = 0;
    for (int p = 0; p <= count; ++p) {
      if (p < count && (V[p] > SAMPLE_ONCHIP) == (large != 0)) {
        ScoreProblem& q = sb.p[n++];
        q.logits = logits[p];
        q.row_stride = row_stride[p];
        q.tok = tok[p];
        q.tok_stride = tok_stride[p];
        q.logprob = logprob[p];
        q.lp_stride = lp_stride[p];
        q.V = V[p];
      }
      if (n == MMT_MAX_GROUP || (p == count && n > 0)) {
        for (int k = n; k < MMT_MAX_GROUP; ++k) sb.p[k] = sb.p[0];  // never read: grid.y == n
        const dim3 grid((unsigned)batch, (unsigned)n);
        if (large)
          hipLaunchKernelGGL(score_multi_kernel<false>, grid, dim3(SAMPLE_THREADS), 0, s, sb);
        else
          hipLaunchKernelGGL(score_multi_kernel<true>, grid, dim3(SAMPLE_THREADS), 0, s, sb);
        if (hipGetLastError() != hipSuccess) return MMT_ERR_HIP;
        n = 0;
      }
    }
  }
  return MMT_OK;
}

}  // extern "C"
