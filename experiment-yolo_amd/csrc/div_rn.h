// The correctly rounded fp32 quotient x / s from the host's correctly rounded reciprocal rs = 1 / s (two fma corrections, Markstein's
// theorem; finite, normal operands), shared by tta.hip and tiled.hip.  The pragma is function-local: including this header leaves
// the contraction mode of the including file as it was.
#pragma once

static __device__ __forceinline__ float div_rn(float x, float s, float rs) {
#pragma clang fp contract(off)
  const float q = x * rs;
  const float q1 = __builtin_fmaf(__builtin_fmaf(-q, s, x), rs, q);
  return __builtin_fmaf(__builtin_fmaf(-q1, s, x), rs, q1);
}
