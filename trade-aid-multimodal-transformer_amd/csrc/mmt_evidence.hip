// Evidence of conditioned rollouts (mmt.h: mmt_resample, mmt_fanout_gather): the particle-filter step over the S
// paths of a prompt, and the row gather that moves the fan-out tails to their ancestors.
//
// mmt_resample: one 256-thread workgroup per prompt, nothing shared between prompts. The S log-weights (fp64) and
// weights (fp32) of the prompt stay in LDS (48 KiB at S = 4096, the largest fan; above that MMT_ERR_UNSUPPORTED).
// No float atomics; every sum runs over a fixed assignment and a fixed tree, the sampler's (mmt_sample.hip): thread
// t owns the chunk [t c, t c + c), c = ceil(S / 256) | 1, serial sum, shift scan over the lanes, wave totals added
// left to right. So a launch is bit-identical run to run and a prompt gives the same bits alone or in company.
//
// Systematic resampling reads the inclusive prefix sums of that tree from LDS: slot s bisects them for the first
// row that reaches (s + u) / S * W and then skips rows of weight 0, so a dead path is never an ancestor. (Across a
// chunk boundary the tree's prefix may step back by an ulp; the bisection's answer is the rule there.)
#include "mmt.h"
#include "mmt_common.h"
#include "mmt_kernels.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / MMT_WAVE;
constexpr int RS_MAX_S = 4096;
constexpr uint32_t RS_SALT = 0x52534D50u;  // "RSMP"

struct ResampleInputs {
  const float* lp[MMT_MAX_GROUP];
  int64_t stride[MMT_MAX_GROUP];
  int count;
};

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(
    ResampleInputs in, int S, int j0, int j1, double* __restrict__ logw, double* __restrict__ log_evidence,
    double ess_threshold, int fold, uint32_t key, uint32_t pos, int32_t* __restrict__ ancestors,
    int32_t* __restrict__ resampled) {
  __shared__ double ps[RS_MAX_S];  // a_s, then the inclusive prefix sums of e
  __shared__ float es[RS_MAX_S];
  __shared__ double shd[3][RS_WAVES];
  __shared__ int shi[RS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int64_t r0 = (int64_t)b * S;

  // step 1: a_s = logw + the columns j0..j1-1 of the given modalities, serial; NaN as -inf
  double mx = -INFINITY;
  for (int s = tid; s < S; s += RS_THREADS) {
    const int64_t r = r0 + s;
    double a = logw[r];
    if (a != a) a = -INFINITY;
    for (int j = j0; j < j1; ++j)
      for (int g = 0; g < in.count; ++g) {
        double t = (double)in.lp[g][r * in.stride[g] + j];
        if (t != t) t = -INFINITY;
        a += t;
      }
    if (a != a) a = -INFINITY;  // +inf - inf: no weight either
    ps[s] = a;
    mx = fmax(mx, a);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) shd[0][wave] = mx;
  __syncthreads();
  mx = fmax(fmax(shd[0][0], shd[0][1]), fmax(shd[0][2], shd[0][3]));

  if (mx == -INFINITY) {  // no live path (uniform branch); every thread reads back its own ps entries
    for (int s = tid; s < S; s += RS_THREADS) {
      logw[r0 + s] = ps[s];
      ancestors[r0 + s] = (int32_t)(r0 + s);
    }
    if (tid == 0) {
      resampled[b] = 0;
      if (fold) log_evidence[b] += -INFINITY;
    }
    return;
  }

  // step 2: fp32 weights, W and Q in fp64 over the chunk tree
  for (int s = tid; s < S; s += RS_THREADS) {
    const float d = (float)(ps[s] - mx);
    es[s] = d == 0.f ? 1.0f : expf(d);
  }
  __syncthreads();
  const int c = ((S + RS_THREADS - 1) / RS_THREADS) | 1;
  const int i0 = min(tid * c, S), i1 = min(tid * c + c, S);
  double totW = 0.0, totQ = 0.0;
  int lastlive = -1;
  for (int i = i0; i < i1; ++i) {
    const double w = (double)es[i];
    totW += w;
    totQ += w * w;  // the product of two fp32 values is exact in fp64
    if (es[i] > 0.f) lastlive = i;
  }
  double incW = totW, incQ = totQ;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double nW = __shfl_up(incW, o, 64), nQ = __shfl_up(incQ, o, 64);
    if (lane >= o) { incW += nW; incQ += nQ; }
  }
  double exW = __shfl_up(incW, 1, 64);
  if (lane == 0) exW = 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lastlive = max(lastlive, __shfl_xor(lastlive, o, 64));
  if (lane == 63) { shd[1][wave] = incW; shd[2][wave] = incQ; }
  if (lane == 0) shi[wave] = lastlive;
  __syncthreads();
  const double w0 = shd[1][0], w1 = shd[1][1], w2 = shd[1][2], w3 = shd[1][3];
  const double W = ((w0 + w1) + w2) + w3;
  const double Q = ((shd[2][0] + shd[2][1]) + shd[2][2]) + shd[2][3];
  lastlive = max(max(shi[0], shi[1]), max(shi[2], shi[3]));
  const double ess = W * W / Q;
  const bool trigger = !fold && ess < ess_threshold * (double)S;

  if (!trigger) {  // step 3 (uniform branch); ps still holds a_s, every thread reads its own entries
    for (int s = tid; s < S; s += RS_THREADS) {
      logw[r0 + s] = ps[s];
      ancestors[r0 + s] = (int32_t)(r0 + s);
    }
    if (tid == 0) {
      resampled[b] = 0;
      if (fold) log_evidence[b] += mx + log(W / (double)S);
    }
    return;
  }

  // step 4: the inclusive prefix sums (every read of a_s happened before the barrier above), then one bisection
  // per slot
  {
    const double wbase = wave == 0 ? 0.0 : wave == 1 ? w0 : wave == 2 ? (w0 + w1) : ((w0 + w1) + w2);
    double p = wbase + exW;
    for (int i = i0; i < i1; ++i) {
      p += (double)es[i];
      ps[i] = p;
    }
  }
  __syncthreads();
  const uint32_t h = mmt_hash(key, (uint32_t)b, pos);
  const double u = ((double)(h >> 8) + 0.5) * (1.0 / 16777216.0);
  for (int s = tid; s < S; s += RS_THREADS) {
    const double target = ((double)s + u) / (double)S * W;
    int lo = 0, hi = S;  // the first i in [0, S) with ps[i] >= target, S when there is none
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ps[mid] >= target) hi = mid; else lo = mid + 1;
    }
    while (lo < S && !(es[lo] > 0.f)) ++lo;
    if (lo >= S) lo = lastlive;
    ancestors[r0 + s] = (int32_t)(r0 + lo);
    logw[r0 + s] = 0.0;
  }
  if (tid == 0) {
    log_evidence[b] += mx + log(W / (double)S);
    resampled[b] = 1;
  }
}

__global__ __launch_bounds__(256) void row_gather_kernel(GatherBatch g, const int32_t* __restrict__ anc, int rows) {
  const GatherSeg& q = g.seg[blockIdx.z];
  const int r = blockIdx.x;
  int a = anc[r];
  if ((unsigned)a >= (unsigned)rows) a = r;
  const int64_t off = ((int64_t)blockIdx.y * 256 + threadIdx.x) * 16;
  if (off < q.bytes)
    *reinterpret_cast<u32x4*>(q.dst + (int64_t)r * q.row_bytes + off) =
        *reinterpret_cast<const u32x4*>(q.src + (int64_t)a * q.row_bytes + off);
}

}  // namespace

hipError_t mmt_launch_row_gather(const GatherBatch& b, const int32_t* anc, int rows, hipStream_t s) {
  if (b.count == 0 || rows == 0) return hipSuccess;
  if (b.count < 0 || b.count > MMT_GATHER_SEGS || rows < 0 || !anc) return hipErrorInvalidValue;
  int64_t most = 0;
  for (int i = 0; i < b.count; ++i) {
    const GatherSeg& q = b.seg[i];
    if (!q.src || !q.dst || q.bytes < 0 || q.bytes > q.row_bytes || ((q.bytes | q.row_bytes) & 15) ||
        (((uintptr_t)q.src | (uintptr_t)q.dst) & 15))
      return hipErrorInvalidValue;
    most = q.bytes > most ? q.bytes : most;
  }
  const int64_t chunks = (most + 4095) / 4096;
  if (chunks == 0) return hipSuccess;
  if (chunks > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(row_gather_kernel, dim3((unsigned)rows, (unsigned)chunks, (unsigned)b.count), dim3(256), 0, s, b,
                     anc, rows);
  return hipGetLastError();
}

extern "C" int mmt_resample(void* stream, int32_t batch, int32_t samples, int32_t count, const float* const* logprob,
                            const int64_t* lp_stride, int32_t j0, int32_t j1, double* logw, double* log_evidence,
                            double ess_threshold, uint64_t seed, uint32_t pos, int32_t* ancestors,
                            int32_t* resampled) {
  if (batch < 0 || samples < 1 || count < 0 || count > MMT_MAX_GROUP || j0 < 0 || j1 < j0 ||
      ess_threshold != ess_threshold)
    return MMT_ERR_INVALID;
  if (count > 0 && j1 > j0 && (!logprob || !lp_stride)) return MMT_ERR_INVALID;
  if ((int64_t)batch * samples > 0x7fffffff) return MMT_ERR_INVALID;  // ancestors are int32 row indices
  ResampleInputs in{};
  in.count = j1 > j0 ? count : 0;
  for (int g = 0; g < in.count; ++g) {
    if (batch > 0 && !logprob[g]) return MMT_ERR_INVALID;
    if (lp_stride[g] < j1) return MMT_ERR_INVALID;
    in.lp[g] = logprob[g];
    in.stride[g] = lp_stride[g];
  }
  if (batch > 0 && (!logw || !log_evidence || !ancestors || !resampled)) return MMT_ERR_INVALID;
  if (samples > RS_MAX_S) return MMT_ERR_UNSUPPORTED;
  if (batch == 0) return MMT_OK;
  const int fold = ess_threshold < 0.0 ? 1 : 0;
  const uint32_t key = mmt_hash((uint32_t)seed, (uint32_t)(seed >> 32), RS_SALT);
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)batch), dim3(RS_THREADS), 0, (hipStream_t)stream, in, samples,
                     j0, j1, logw, log_evidence, ess_threshold, fold, key, pos, ancestors, resampled);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_ERR_HIP;
}
