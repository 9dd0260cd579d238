// One bounding op with a slope (layers/bounding.py; include/anemoi_amd.h: anemoi_bound_output_leaky), shared by the inference
// kernel (csrc/elementwise.hip, LEAKY) and the training pair (csrc/bounding.hip).
#pragma once

#include "common.hpp"

namespace anemoi {

// f(v) = lo + s (v - lo) below lo, hi + s (v - hi) above hi, v between them.  Comparisons (not fminf / fmaxf): a NaN fails
// both and stays a NaN.  s == 0 selects the bound itself -- the hard classes' clamp, bit for bit, also for v = -inf / +inf
// (0 * inf would be a NaN).
__device__ __forceinline__ float bound_op(float v, float lo, float hi, float s) {
  if (v < lo) return s == 0.f ? lo : lo + s * (v - lo);
  if (v > hi) return s == 0.f ? hi : hi + s * (v - hi);
  return v;
}

// f'(v): 1 strictly inside (lo, hi), s elsewhere -- AT a bound the slope is s, which is what torch's relu (0 at 0) and
// hardtanh (0 at min_val and max_val) backward give for the hard classes.  (A NaN is inside no interval: s.)
__device__ __forceinline__ float bound_op_grad(float v, float lo, float hi, float s) {
  return (v > lo && v < hi) ? 1.f : s;
}

}  // namespace anemoi
