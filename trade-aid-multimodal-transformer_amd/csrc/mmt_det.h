// Deterministic training mode (mmt_set_deterministic): per-block partial sums + one ordered sum.
//
// Every kernel of the backward that adds a block's column sums into a gradient with one float atomic
// per element (arrival order: the low bits change run to run) takes a nullable scratch pointer. With it
// set, the block STORES its sums at
//     base + problem * stride + (destination region) + partial * n + element
// where `partial` is the block's LOGICAL row-tile index (never blockIdx: the launches remap blocks
// across XCDs) and `element` the index the atomic would have used inside the destination, and the
// launcher queues ordered_sum_kernel right behind the producer on the same stream:
//     acc = parts[0]; acc = acc + parts[k] (k = 1 .. nparts - 1, index order); dst = dst + acc
// The launcher zeroes the region it is about to use before the producer runs, so a slot no block of
// this launch writes (a tile taller than the 128-row partial unit, a block that exits early) adds an
// exact +0 and the sum never reads what an earlier launch left there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef MMT_MAX_GROUP
#define MMT_MAX_GROUP 8
#endif

// one destination vector of one problem: dst[i] += ordered sum over k of parts[k * ld + i], i < n
struct DetSeg {
  float* dst;
  const float* parts;
  int64_t ld;
  int nparts, n;
};
#define MMT_DET_MAX_SEG (3 * MMT_MAX_GROUP)
struct DetSumBatch {
  DetSeg s[MMT_DET_MAX_SEG];
  int count;
};
hipError_t mmt_launch_ordered_sum(const DetSumBatch& b, hipStream_t s);

// the producers' side, one per *Batch struct. base == nullptr: the default (atomic) path.
struct DetScratch {
  float* base;     // device scratch (16-B aligned)
  int64_t stride;  // floats per problem (set by the launcher)
  int64_t cap;     // floats available at base (host side)
  // host side, optional: called with 0 before and 1 after the ordered-sum launch (the engine's probe)
  void (*hook)(void* user, int after);
  void* user;
};

// host helper of the launchers: region bookkeeping of one producer launch
struct DetLaunch {
  DetSumBatch sb{};
  const DetScratch* d = nullptr;
  hipStream_t s = nullptr;
  // claims count * stride floats and zeroes them; hipErrorInvalidValue when the scratch is too small
  // (the caller then fails the step: a deterministic launch never falls back to the atomics)
  hipError_t begin(const DetScratch& ds, int count, int64_t stride, hipStream_t st) {
    d = &ds; s = st; sb.count = 0;
    const int64_t need = (int64_t)count * stride;
    if (need > ds.cap || ((uintptr_t)ds.base & 15)) return hipErrorInvalidValue;
    if (need == 0) return hipSuccess;
    return hipMemsetAsync(ds.base, 0, (size_t)need * sizeof(float), st);
  }
  // problem g's destination `dst` (null: skipped) with its partials at float offset `off` of the problem
  void seg(int g, int64_t stride, int64_t off, float* dst, int nparts, int n) {
    if (!dst || nparts <= 0 || n <= 0) return;
    DetSeg& q = sb.s[sb.count++];
    q.dst = dst; q.parts = d->base + (int64_t)g * stride + off; q.ld = n; q.nparts = nparts; q.n = n;
  }
  hipError_t finish() {
    if (sb.count == 0) return hipSuccess;
    if (d->hook) d->hook(d->user, 0);
    const hipError_t e = mmt_launch_ordered_sum(sb, s);
    if (d->hook) d->hook(d->user, 1);
    return e;
  }
};

// rows of the GEMM epilogues' partial unit: every tile is 128 or 256 rows tall, a block's partial index is
// m0 / BM, and the launcher sums ceil(M / 128) slots (the unused ones hold the launcher's zeros)
#define MMT_DET_GEMM_ROWS 128
