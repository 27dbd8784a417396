// Device helpers shared by the evaluation kernels (mmt_evalpos.hip, mmt_evaltemp.hip): the NaN a dead row holds, the
// direction sign of a token and the bin of a probability. One definition, so the two entries agree on every class
// and every bin.
#pragma once
#include "mmt_common.h"

namespace {

__device__ __forceinline__ double ev_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the reference's _get_direction_sign: of the value itself (percent) or of value - value[xb]
__device__ __forceinline__ int ev_sign(double v, double vo, int pct) {
  const double ch = pct ? v : v - vo;
  return ch > 0.0 ? 1 : (ch < 0.0 ? -1 : 0);
}

__device__ __forceinline__ int ev_bin(double p, int bins) {
  const int k = (int)floor(p * (double)bins);
  return k < bins - 1 ? k : bins - 1;
}

}  // namespace
