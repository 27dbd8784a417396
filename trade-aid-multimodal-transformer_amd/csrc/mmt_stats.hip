// Per-tensor statistics of a flat fp32 buffer and the first-fault record (mmt.h: mmt_tensor_stats).
//
// Three launches on the caller's stream, in the manner of the guard kernels of mmt_elem.hip (fp64 from the
// per-thread accumulator on, fixed trees, plain stores, no float atomics, no workgroup waits for another):
//   stats_partial_kernel  one workgroup per MMT_STATS_CHUNK elements, one wave per quarter of the chunk, 16-byte
//                         loads. A wave whose quarter lies inside one segment (the streaming case) sums it with a
//                         plain xor tree. Otherwise every lane turns 16 consecutive elements into a RUN SUMMARY: the
//                         partial of its first run (a run = consecutive elements of one segment), the partial of
//                         its last run, and their segment keys. Two neighbouring summaries combine into one: the
//                         runs that meet in the middle are added when they share a key, and a run that is now
//                         enclosed on both sides is complete for this chunk and is stored at once. The wave
//                         combines its 64 lanes in a fixed shuffle tree, thread 0 chains the four waves through
//                         LDS and stores the two runs that are left. A complete run
//                         of (chunk c, segment s) goes to scratch slot c + s: along the ordered list of
//                         overlapping (chunk, segment) pairs c + s is strictly increasing, so no two pairs share
//                         a slot and every slot index is below nchunks + nseg.
//   stats_segment_kernel  one wave per segment: lane l adds the slots of chunks c_lo + l, c_lo + l + 64, ... in
//                         that order, then a fixed xor tree; one mmt_tensor_stat per segment.
//   stats_commit_kernel   one thread: the header (counters from the guard, valid = 1).
// In mode MMT_STATS_ON_SKIP every workgroup of the three launches first loads the guard's `ok` and the
// record's `valid` and returns unless ok == 0 and valid == 0. Only the commit launch writes `valid`, after
// the other two have finished (stream order), so all of them decide alike and a clean step never reads x.
// Segment offsets are clamped to [0, n] and segment keys to [-1, nseg] (both ends: "no segment"), so no table
// content, sorted or not, takes an access out of x, the scratch or the record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mmt.h"
#include "mmt_common.h"

static_assert(sizeof(mmt_tensor_stat) == 40, "mmt_tensor_stat is 40 bytes (mmt_lib.MmtTensorStat)");
static_assert(sizeof(mmt_stats_header) == 32, "mmt_stats_header is 32 bytes (mmt_lib.MmtStatsHeader)");

namespace {

constexpr int STATS_THREADS = 256;
constexpr int STATS_WAVES = STATS_THREADS / 64;
constexpr int WAVE_ELEMS = MMT_STATS_CHUNK / STATS_WAVES;  // elements of a chunk one wave reads
constexpr int WAVE_PASSES = WAVE_ELEMS / 256;              // 16-byte loads per lane
constexpr int LANE_ELEMS = WAVE_ELEMS / 64;                // consecutive elements of a lane off the streaming path
constexpr int LANE_VECS = LANE_ELEMS / 4;
static_assert(WAVE_ELEMS % 256 == 0 && WAVE_PASSES >= 1, "a wave reads whole passes of 64 x 16 bytes");
constexpr int NO_BAD = 0x7fffffff;

// statistics of some elements of one segment inside one chunk; fb = position in the chunk of the first
// non-finite one
struct Part {
  double sq;
  float amax;
  int nan, inf, fb;
};
struct alignas(16) Slot {  // a Part as the scratch holds it; fb = index inside the segment
  double sq;
  int64_t fb;
  int32_t nan, inf;
  float amax;
  int32_t pad;
};
static_assert(sizeof(Slot) == 32, "mmt_stats_scratch_bytes counts 32-byte slots");
// run summary of a range of elements: a = its first run (key k0), b = its last run (key k1); k0 == k1: one
// run, held in a
struct Summ {
  Part a, b;
  int k0, k1;
};
struct Tab {
  const int64_t* b;
  int nseg;
  int64_t n;
};

__device__ __forceinline__ Part part_zero() { return Part{0.0, 0.f, 0, 0, NO_BAD}; }
__device__ __forceinline__ void part_add(Part& p, const Part& q) {
  p.sq += q.sq;
  p.amax = fmaxf(p.amax, q.amax);
  p.nan += q.nan;
  p.inf += q.inf;
  p.fb = p.fb < q.fb ? p.fb : q.fb;
}
__device__ __forceinline__ void part_elem(Part& p, float x, int pos) {
  const uint32_t bits = __float_as_uint(x);
  if ((bits & 0x7f800000u) != 0x7f800000u) {
    const double d = (double)x;
    p.sq += d * d;  // the square of an fp32 value is exact in fp64
    p.amax = fmaxf(p.amax, fabsf(x));
  } else {
    if (bits & 0x007fffffu) p.nan += 1; else p.inf += 1;
    p.fb = p.fb < pos ? p.fb : pos;
  }
}
__device__ __forceinline__ Part part_shfl_xor(const Part& p, int o) {
  return Part{__shfl_xor(p.sq, o, 64), __shfl_xor(p.amax, o, 64), __shfl_xor(p.nan, o, 64), __shfl_xor(p.inf, o, 64),
              __shfl_xor(p.fb, o, 64)};
}
__device__ __forceinline__ Part part_shfl_down(const Part& p, int o) {
  return Part{__shfl_down(p.sq, o, 64), __shfl_down(p.amax, o, 64), __shfl_down(p.nan, o, 64),
              __shfl_down(p.inf, o, 64), __shfl_down(p.fb, o, 64)};
}
__device__ __forceinline__ Summ summ_one(int k, const Part& p) { return Summ{p, part_zero(), k, k}; }

// entry i of the table (0 <= i <= nseg), clamped to [0, n]
__device__ __forceinline__ int64_t tab_at(const Tab& t, int i) {
  const int64_t v = t.b[i];
  return v < 0 ? 0 : (v > t.n ? t.n : v);
}
// first element past the run of key k
__device__ __forceinline__ int64_t tab_next(const Tab& t, int k) { return k >= t.nseg ? INT64_MAX : tab_at(t, k + 1); }

// a run that is complete for chunk c: one plain 32-byte store
__device__ __forceinline__ void flush(const Tab& t, Slot* scratch, int64_t c, int key, const Part& p) {
  if (key < 0 || key >= t.nseg) return;  // elements of no segment
  Slot s;
  s.sq = p.sq;
  s.fb = p.fb == NO_BAD ? INT64_MAX : c * MMT_STATS_CHUNK + p.fb - tab_at(t, key);
  s.nan = p.nan;
  s.inf = p.inf;
  s.amax = p.amax;
  s.pad = 0;
  scratch[c + key] = s;
}

// summary of the range L covers followed by the range R covers; `live` = this lane's result is used, so
// it stores the runs that the combination encloses
__device__ __forceinline__ Summ combine(const Summ& L, const Summ& R, bool live, const Tab& t, Slot* scratch, int64_t c) {
  const bool l2 = L.k0 != L.k1, r2 = R.k0 != R.k1;
  Summ out;
  out.k0 = L.k0;
  out.k1 = R.k1;
  if (L.k1 == R.k0) {
    Part m = l2 ? L.b : L.a;
    part_add(m, R.a);
    if (!l2 && !r2) {
      out.a = m;
      out.b = part_zero();
    } else if (!l2) {
      out.a = m;
      out.b = R.b;
    } else if (!r2) {
      out.a = L.a;
      out.b = m;
    } else {
      if (live) flush(t, scratch, c, L.k1, m);
      out.a = L.a;
      out.b = R.b;
    }
  } else {
    if (live && l2) flush(t, scratch, c, L.k1, L.b);
    if (live && r2) flush(t, scratch, c, R.k0, R.a);
    out.a = L.a;
    out.b = r2 ? R.b : R.a;
  }
  return out;
}

// the segment of element idx: (entries <= idx) - 1, so -1 below the table, nseg from its last entry on, and
// an empty segment is never the answer. idx is wave-uniform and all 64 lanes are active: a 64-ary search, two
// or three rounds of one load per lane instead of a dozen dependent ones
__device__ __forceinline__ int tab_find_wave(const Tab& t, int64_t idx, int lane) {
  int lo = 0, hi = t.nseg + 1;  // entries [0, lo) are <= idx, entries [hi, nseg] are > idx
  while (lo < hi) {
    const int s = (hi - lo + 63) / 64;
    const int p = lo + lane * s;
    const bool le = p < hi && tab_at(t, p) <= idx;
    const int cnt = __popcll(__ballot(le));  // a prefix of the lanes: the table ascends
    if (cnt == 0) {
      hi = lo;
    } else {
      const int up = lo + cnt * s;
      lo = lo + (cnt - 1) * s + 1;
      hi = up < hi ? up : hi;
    }
  }
  return lo - 1;
}
// the same, per lane, for an element at or past the first element of segment k0 (k0 = -1: anywhere): probes
// k0 + 1, k0 + 2, k0 + 4, ... before it bisects, so a neighbouring segment costs one or two loads
__device__ __forceinline__ int tab_find_from(const Tab& t, int64_t idx, int k0) {
  int lo = k0 + 1, hi = t.nseg + 1;
  if (lo < 0) lo = 0;
  for (int w = 1; lo < hi; w <<= 1) {
    int p = lo + w - 1;
    if (p >= hi) p = hi - 1;
    if (tab_at(t, p) <= idx) {
      lo = p + 1;
    } else {
      hi = p;
      break;
    }
  }
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab_at(t, mid) <= idx) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// the LANE_ELEMS consecutive elements from idx0 on (pos0 = their position in the chunk, kw = a segment at or
// below theirs); a run that begins and ends inside them is complete and stored here
__device__ __forceinline__ Summ lane_summary(const Tab& t, const float* x, int64_t idx0, int pos0, int kw, Slot* scratch,
                                             int64_t c) {
  if (idx0 >= t.n) return summ_one(t.nseg, part_zero());
  int k = tab_find_from(t, idx0, kw);
  int64_t nb = tab_next(t, k);
  Summ S = summ_one(k, part_zero());
  Part cur = part_zero();
  int closed = 0;
#pragma unroll
  for (int j = 0; j < LANE_VECS; ++j) {
    const int64_t base = idx0 + 4 * j;
    if (base >= t.n) break;
    float v[4];
    int cnt = 4;
    if (base + 4 <= t.n) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(x + base);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = q[e];
    } else {  // the buffer's last, partial vector
      cnt = (int)(t.n - base);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = e < cnt ? x[base + e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < cnt) {
        const int64_t idx = base + e;
        if (idx >= nb) {  // a segment head or tail off the 4-boundary: the run of key k ends before idx
          if (closed == 0) {
            S.k0 = k;
            S.a = cur;
          } else {
            flush(t, scratch, c, k, cur);
          }
          ++closed;
          cur = part_zero();
          k = tab_find_from(t, idx, k);
          nb = tab_next(t, k);
        }
        part_elem(cur, v[e], pos0 + 4 * j + e);
      }
    }
  }
  if (closed == 0) {
    S.k0 = S.k1 = k;
    S.a = cur;
  } else {
    S.k1 = k;
    S.b = cur;
  }
  return S;
}

__device__ __forceinline__ bool stats_idle(int mode, const mmt_guard_header* guard, const mmt_stats_header* rec) {
  return mode == MMT_STATS_ON_SKIP && (guard->ok != 0 || rec->valid != 0);
}

__global__ __launch_bounds__(STATS_THREADS) void stats_partial_kernel(const float* x, int64_t n, const int64_t* seg_begin,
                                                                      int nseg, int mode, const mmt_guard_header* guard,
                                                                      const mmt_stats_header* rec, Slot* scratch) {
  if (stats_idle(mode, guard, rec)) return;  // workgroup-uniform
  __shared__ Summ sh[STATS_WAVES];
  const Tab t{seg_begin, nseg, n};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c = blockIdx.x;
  const int64_t wb = c * MMT_STATS_CHUNK + (int64_t)wave * WAVE_ELEMS;
  Summ W;
  if (wb >= n) {
    W = summ_one(nseg, part_zero());
  } else {
    const int kw = tab_find_wave(t, wb, lane);  // wave-uniform
    if (wb + WAVE_ELEMS <= n && tab_next(t, kw) >= wb + WAVE_ELEMS) {
      // the streaming path: the wave's whole range belongs to segment kw (or to none: nothing to read)
      Part p = part_zero();
      if (kw >= 0 && kw < nseg) {
        f32x4 v[WAVE_PASSES];
#pragma unroll
        for (int j = 0; j < WAVE_PASSES; ++j) v[j] = reinterpret_cast<const f32x4*>(x + wb)[j * 64 + lane];
#pragma unroll
        for (int j = 0; j < WAVE_PASSES; ++j) {
#pragma unroll
          for (int e = 0; e < 4; ++e) part_elem(p, v[j][e], wave * WAVE_ELEMS + j * 256 + lane * 4 + e);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {  // the same tree in every lane
          const Part q = part_shfl_xor(p, o);
          part_add(p, q);
        }
      }
      W = summ_one(kw, p);
    } else {
      // a segment boundary in the wave's range: every lane takes LANE_ELEMS consecutive elements
      const int pos0 = wave * WAVE_ELEMS + lane * LANE_ELEMS;
      W = lane_summary(t, x, c * MMT_STATS_CHUNK + pos0, pos0, kw, scratch, c);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {  // lane l takes lanes [l, l + 2 o) when l % (2 o) == 0
        Summ R;
        R.a = part_shfl_down(W.a, o);
        R.b = part_shfl_down(W.b, o);
        R.k0 = __shfl_down(W.k0, o, 64);
        R.k1 = __shfl_down(W.k1, o, 64);
        W = combine(W, R, (lane & (2 * o - 1)) == 0, t, scratch, c);
      }
    }
  }
  if (lane == 0) sh[wave] = W;
  __syncthreads();
  if (threadIdx.x != 0) return;
  Summ B = sh[0];
#pragma unroll
  for (int w = 1; w < STATS_WAVES; ++w) B = combine(B, sh[w], true, t, scratch, c);
  flush(t, scratch, c, B.k0, B.a);
  if (B.k1 != B.k0) flush(t, scratch, c, B.k1, B.b);
}

__global__ __launch_bounds__(STATS_THREADS) void stats_segment_kernel(int64_t n, const int64_t* seg_begin, int nseg,
                                                                      int mode, const mmt_guard_header* guard,
                                                                      const mmt_stats_header* rec, const Slot* scratch,
                                                                      mmt_tensor_stat* out) {
  if (stats_idle(mode, guard, rec)) return;
  const Tab t{seg_begin, nseg, n};
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * STATS_WAVES + (threadIdx.x >> 6);
  if (s >= nseg) return;  // wave-uniform
  const int64_t b0 = tab_at(t, s), b1 = tab_at(t, s + 1);
  double sq = 0.0;
  float amax = 0.f;
  int64_t nan = 0, inf = 0, fb = INT64_MAX;
  if (b1 > b0) {
    const int64_t c_lo = b0 / MMT_STATS_CHUNK, c_hi = (b1 - 1) / MMT_STATS_CHUNK;
    for (int64_t c = c_lo + lane; c <= c_hi; c += 64) {  // chunk order within the lane
      const Slot q = scratch[c + s];
      sq += q.sq;
      amax = fmaxf(amax, q.amax);
      nan += q.nan;
      inf += q.inf;
      fb = fb < q.fb ? fb : q.fb;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sq += __shfl_xor(sq, o, 64);
    amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    nan += __shfl_xor((long long)nan, o, 64);
    inf += __shfl_xor((long long)inf, o, 64);
    const int64_t f = __shfl_xor((long long)fb, o, 64);
    fb = fb < f ? fb : f;
  }
  if (lane != 0) return;
  mmt_tensor_stat r;
  r.sqsum = sq;
  r.nan_count = nan;
  r.inf_count = inf;
  r.first_bad = fb == INT64_MAX ? -1 : fb;
  r.absmax = amax;
  r.reserved = 0.f;
  out[s] = r;
}

__global__ __launch_bounds__(64) void stats_commit_kernel(int nseg, int mode, const mmt_guard_header* guard,
                                                          mmt_stats_header* rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (stats_idle(mode, guard, rec)) return;
  rec->nseg = nseg;
  rec->applied_steps = guard ? guard->applied_steps : 0;
  rec->skipped_steps = guard ? guard->skipped_steps : 0;
  rec->reserved = 0;
  rec->valid = 1;
}

bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" {

int64_t mmt_stats_chunk(void) { return MMT_STATS_CHUNK; }

int64_t mmt_stats_record_bytes(int32_t nseg) {
  if (nseg < 0) return -1;
  return (int64_t)sizeof(mmt_stats_header) + (int64_t)nseg * (int64_t)sizeof(mmt_tensor_stat);
}

int64_t mmt_stats_scratch_bytes(int64_t n, int32_t nseg) {
  if (n < 0 || nseg < 0) return -1;
  const int64_t nchunks = (n + MMT_STATS_CHUNK - 1) / MMT_STATS_CHUNK;
  const int64_t slots = nchunks + nseg;  // c + s < nchunks + nseg
  return (slots > 0 ? slots : 1) * (int64_t)sizeof(Slot);
}

int mmt_tensor_stats(void* stream, const float* x, int64_t n, const int64_t* seg_begin, int32_t nseg, int32_t mode,
                     const void* guard, void* scratch, void* record) {
  if (n < 0 || nseg < 0 || (n > 0 && !x) || !seg_begin || !scratch || !record) return MMT_ERR_INVALID;
  if (mode != MMT_STATS_ALWAYS && mode != MMT_STATS_ON_SKIP) return MMT_ERR_INVALID;
  if (mode == MMT_STATS_ON_SKIP && !guard) return MMT_ERR_INVALID;
  if (misaligned16(x) || misaligned16(scratch) || misaligned16(record) || misaligned16(guard)) return MMT_ERR_INVALID;
  const int64_t nchunks = (n + MMT_STATS_CHUNK - 1) / MMT_STATS_CHUNK;
  if (nchunks > 0x7fffffff) return MMT_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const mmt_guard_header* g = static_cast<const mmt_guard_header*>(guard);
  mmt_stats_header* rec = static_cast<mmt_stats_header*>(record);
  mmt_tensor_stat* out = reinterpret_cast<mmt_tensor_stat*>(static_cast<char*>(record) + sizeof(mmt_stats_header));
  if (nseg > 0 && nchunks > 0) {
    hipLaunchKernelGGL(stats_partial_kernel, dim3((unsigned)nchunks), dim3(STATS_THREADS), 0, s, x, n, seg_begin, nseg,
                       mode, g, rec, static_cast<Slot*>(scratch));
    if (hipGetLastError() != hipSuccess) return MMT_ERR_HIP;
  }
  if (nseg > 0) {
    hipLaunchKernelGGL(stats_segment_kernel, dim3((unsigned)((nseg + STATS_WAVES - 1) / STATS_WAVES)),
                       dim3(STATS_THREADS), 0, s, n, seg_begin, nseg, mode, g, rec, static_cast<const Slot*>(scratch),
                       out);
    if (hipGetLastError() != hipSuccess) return MMT_ERR_HIP;
  }
  hipLaunchKernelGGL(stats_commit_kernel, dim3(1), dim3(64), 0, s, nseg, mode, g, rec);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_ERR_HIP;
}

}  // extern "C"
