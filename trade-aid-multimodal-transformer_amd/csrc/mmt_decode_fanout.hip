// Sample fan-out decode attention (generate with num_samples = S): S continuations of one prompt share the
// prompt's keys / values. Row r = b*S + s of the compact query / output is sample s of prompt b; positions
// 0..n0-1 (the prefix) are the workspace cache rows b*T + p the prefill left, positions n0..t each sample's own
// tail rows r*tail_rows + (p - n0). One softmax per KV stream over the n = t + 1 keys, the outputs summed, as
// attn_decode_kernel.
//
// One 256-thread workgroup per (prompt, head, problem) and group of FAN_G = 16 samples; the 16 lanes
// [16 sl, 16 sl + 16) of a wave own sample sl of the group: its running maximum m, sum l and, lane kl, the output
// dims kl + 16 c. The prefix is walked once per GROUP in tiles of FAN_KT = 64 keys: the tile's K / V rows are
// fetched once (16-B loads), widened to fp32 in LDS and read by all 16 samples; lane kl scores keys kl + 16 c of
// the tile against its sample's query (fp32 registers), the 16 lanes reduce the tile's maximum and sum by xor
// butterflies, rescale (m, l, acc) by exp(m_old - m_new) and add the tile's p v. The tail follows in the same
// running state, per sample, 64 keys at a time straight from memory. Scores and probabilities are fp32 on the
// VALU, the output is rounded once. No atomics; nothing a sample computes depends on the other samples of its
// group (a short last group recomputes sample S - 1 in its idle lanes and stores nothing for them).
//
// The rolling-window step (generate with rolling=True, mmt_rolling_step) has m tail rows per sample and needs the
// attention of ALL of them: attn_rolling_fanout_kernel is the same body (fanout_body) with the tail position i in
// blockIdx.y, query / output row r*m + i, the prefix n0 = p and i + 1 tail keys: one launch for the m positions, and
// per query the bits of attn_decode_fanout_kernel at n0 = p, t = p + i.
#include "mmt_common.h"
#include "mmt_kernels.h"

#define FAN_G MMT_FANOUT_G
#define FAN_KT 64

namespace {

__device__ __forceinline__ float max16(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one tile's four scores of a lane merged into the sample's running state; the probabilities go to ps[kl + 16 c]
template <int NC>
__device__ __forceinline__ void merge_tile(const float (&sc)[4], float& m, float& l, float (&acc)[NC], float* ps,
                                           int kl) {
  const float mn = fmaxf(m, max16(fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]))));
  const float alpha = __expf(m - mn);  // first tile: m = -inf, alpha = 0 on l = acc = 0
  float p[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    p[c] = __expf(sc[c] - mn);  // a key past the tile's end has sc = -inf: p = 0
    ps[kl + 16 * c] = p[c];
  }
  l = l * alpha + sum16(((p[0] + p[1]) + p[2]) + p[3]);
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] *= alpha;
  m = mn;
}

}  // namespace

// The body both kernels run: one workgroup, its group of samples, n0 prefix keys and nt tail keys. Sample row r
// reads query row r * qo_rows + qo_at, the tail rows r * tail_rows + 0..nt-1, and writes output row
// r * qo_rows + qo_at (the fan-out step: qo_rows = 1, qo_at = 0; the rolling step: qo_rows = tail_rows = m,
// qo_at = the tail position, nt = qo_at + 1).
template <int HS>
__device__ __forceinline__ void fanout_body(const FanoutAttnProblem& P, int S, int n0, int nt, int T, int H,
                                            int tail_rows, int qo_rows, int qo_at, float scale) {
  constexpr int NC = (HS + 15) / 16, LDK = HS + 4, CH = HS / 8;
  const int ngrp = (S + FAN_G - 1) / FAN_G;
  const int grp = blockIdx.x % ngrp, bh = blockIdx.x / ngrp, b = bh / H, head = bh % H;
  const int tid = threadIdx.x, sl = tid >> 4, kl = tid & 15;
  const bool live = grp * FAN_G + sl < S;
  const int64_t r = (int64_t)b * S + (live ? grp * FAN_G + sl : S - 1);
  __shared__ __attribute__((aligned(16))) float Ks[FAN_KT * LDK];
  __shared__ __attribute__((aligned(16))) float Vs[FAN_KT * HS];
  __shared__ __attribute__((aligned(16))) float Ps[FAN_G * FAN_KT];
  float* ps = Ps + sl * FAN_KT;
  float q[HS];
  {
    const bf16_t* qp = P.q + (r * qo_rows + qo_at) * P.q_ld + head * HS;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(qp + 8 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        q[8 * c + 2 * e] = bf2f(v[e] & 0xffff) * scale;
        q[8 * c + 2 * e + 1] = bf2f(v[e] >> 16) * scale;
      }
    }
  }
  float o[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) o[c] = 0.f;
  for (int j = 0; j < P.nstreams; ++j) {
    float m = -INFINITY, l = 0.f, acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.f;
    // ---- the shared prefix, once for the group
    const bf16_t* kb = P.k[j] + (int64_t)b * T * P.kv_ld + head * P.kv_hstride;
    const bf16_t* vb = P.v[j] + (int64_t)b * T * P.kv_ld + head * P.kv_hstride;
    for (int k0 = 0; k0 < n0; k0 += FAN_KT) {
      const int kt = min(FAN_KT, n0 - k0);
      __syncthreads();  // the previous tile's readers are done
      for (int i = tid; i < FAN_KT * CH; i += 256) {
        const int row = i / CH, c = i % CH;
        u32x4 kv = {0, 0, 0, 0}, vv = {0, 0, 0, 0};  // rows past the tile's end: zeros (p = 0 times a finite v)
        if (row < kt) {
          kv = *reinterpret_cast<const u32x4*>(kb + (int64_t)(k0 + row) * P.kv_ld + 8 * c);
          vv = *reinterpret_cast<const u32x4*>(vb + (int64_t)(k0 + row) * P.kv_ld + 8 * c);
        }
        float* kd = Ks + row * LDK + 8 * c;
        float* vd = Vs + row * HS + 8 * c;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          kd[2 * e] = bf2f(kv[e] & 0xffff); kd[2 * e + 1] = bf2f(kv[e] >> 16);
          vd[2 * e] = bf2f(vv[e] & 0xffff); vd[2 * e + 1] = bf2f(vv[e] >> 16);
        }
      }
      __syncthreads();
      float sc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float* kr = Ks + (kl + 16 * c) * LDK;
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < HS / 4; ++i) {
          const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + 4 * i);
          a += q[4 * i] * kv[0]; a += q[4 * i + 1] * kv[1]; a += q[4 * i + 2] * kv[2]; a += q[4 * i + 3] * kv[3];
        }
        sc[c] = kl + 16 * c < kt ? a : -INFINITY;
      }
      merge_tile<NC>(sc, m, l, acc, ps, kl);
      __syncthreads();  // ps[] of this sample complete
      for (int k4 = 0; k4 < FAN_KT; k4 += 4) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(ps + k4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const int d = kl + 16 * c < HS ? kl + 16 * c : 0;
            acc[c] += p[e] * Vs[(k4 + e) * HS + d];
          }
      }
    }
    // ---- this sample's own tail, merged into the same running state
    const bf16_t* tk = P.tk[j] + r * tail_rows * P.tail_ld + head * P.kv_hstride;
    const bf16_t* tv = P.tv[j] + r * tail_rows * P.tail_ld + head * P.kv_hstride;
    for (int k0 = 0; k0 < nt; k0 += FAN_KT) {
      const int kt = min(FAN_KT, nt - k0);
      __syncthreads();  // ps[] readers of the previous tile are done
      float sc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int key = kl + 16 * c;
        float a = -INFINITY;
        if (key < kt) {
          const bf16_t* kr = tk + (int64_t)(k0 + key) * P.tail_ld;
          a = 0.f;
#pragma unroll
          for (int i = 0; i < CH; ++i) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(kr + 8 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              a += q[8 * i + 2 * e] * bf2f(v[e] & 0xffff);
              a += q[8 * i + 2 * e + 1] * bf2f(v[e] >> 16);
            }
          }
        }
        sc[c] = a;
      }
      merge_tile<NC>(sc, m, l, acc, ps, kl);
      __syncthreads();
      for (int key = 0; key < kt; ++key) {
        const float p = ps[key];
        const bf16_t* vr = tv + (int64_t)(k0 + key) * P.tail_ld;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int d = kl + 16 * c < HS ? kl + 16 * c : 0;
          acc[c] += p * bf2f(vr[d]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] += acc[c] / l;
  }
  if (live) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (kl + 16 * c < HS) P.o[(r * qo_rows + qo_at) * P.o_ld + head * HS + kl + 16 * c] = f2bf(o[c]);
  }
}

template <int HS>
__global__ __launch_bounds__(256) void attn_decode_fanout_kernel(FanoutAttnBatch batch, int S, int n0, int t, int T,
                                                                 int H, int tail_rows, float scale) {
  fanout_body<HS>(batch.p[blockIdx.z], S, n0, t - n0 + 1 /* tail keys of every sample */, T, H, tail_rows, 1, 0, scale);
}

// Rolling-window step (mmt_rolling_step): every sample has m tail rows and ALL of them are queries. blockIdx.y = i is
// the tail position: query / output row r*m + i against the p prefix keys and the sample's tail rows 0..i, the
// arithmetic of attn_decode_fanout_kernel at n0 = p, t = p + i (same tile walk, same merge order, same bits).
template <int HS>
__global__ __launch_bounds__(256) void attn_rolling_fanout_kernel(FanoutAttnBatch batch, int S, int p, int m, int T,
                                                                  int H, float scale) {
  const int i = blockIdx.y;
  fanout_body<HS>(batch.p[blockIdx.z], S, p, i + 1, T, H, m, m, i, scale);
}

hipError_t mmt_launch_attn_decode_fanout(const FanoutAttnBatch& b, int B, int S, int n0, int t, int T, int H, int hs,
                                         int tail_rows, float scale, hipStream_t s) {
  if (b.count == 0) return hipSuccess;
  if (B < 1 || S < 1 || H < 1 || n0 < 1 || t < n0 || t >= T || t - n0 >= tail_rows) return hipErrorInvalidValue;
  const int64_t wgs = (int64_t)B * H * ((S + FAN_G - 1) / FAN_G);
  if (wgs > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid((unsigned)wgs, 1, b.count);
#define FAN_LAUNCH(HS_) \
  hipLaunchKernelGGL(attn_decode_fanout_kernel<HS_>, grid, dim3(256), 0, s, b, S, n0, t, T, H, tail_rows, scale)
  switch (hs) {
    case 8: FAN_LAUNCH(8); break;
    case 16: FAN_LAUNCH(16); break;
    case 24: FAN_LAUNCH(24); break;
    case 32: FAN_LAUNCH(32); break;
    case 48: FAN_LAUNCH(48); break;
    case 64: FAN_LAUNCH(64); break;
    default: return hipErrorInvalidValue;
  }
#undef FAN_LAUNCH
  return hipGetLastError();
}

hipError_t mmt_launch_attn_rolling_fanout(const FanoutAttnBatch& b, int B, int S, int p, int m, int T, int H, int hs,
                                          float scale, hipStream_t s) {
  if (b.count == 0) return hipSuccess;
  if (B < 1 || S < 1 || H < 1 || p < 1 || m < 1 || (int64_t)p + m > T || m > 65535) return hipErrorInvalidValue;
  const int64_t wgs = (int64_t)B * H * ((S + FAN_G - 1) / FAN_G);
  if (wgs > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid((unsigned)wgs, (unsigned)m, b.count);
#define ROLL_LAUNCH(HS_) \
  hipLaunchKernelGGL(attn_rolling_fanout_kernel<HS_>, grid, dim3(256), 0, s, b, S, p, m, T, H, scale)
  switch (hs) {
    case 8: ROLL_LAUNCH(8); break;
    case 16: ROLL_LAUNCH(16); break;
    case 24: ROLL_LAUNCH(24); break;
    case 32: ROLL_LAUNCH(32); break;
    case 48: ROLL_LAUNCH(48); break;
    case 64: ROLL_LAUNCH(64); break;
    default: return hipErrorInvalidValue;
  }
#undef ROLL_LAUNCH
  return hipGetLastError();
}
