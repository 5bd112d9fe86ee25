// Index and scale helpers of the render MLP's block loop (mlp16s_body.h), as plain functions of
// integers and floats: no HIP types, so a host compiler builds them too (tests/sample_index_check.cpp
// checks them against `/`, `%` and the float division over their whole domain).
#pragma once
#include <stdint.h>
#include "layout.h"

namespace nerf {

// n / d for every 0 <= n < 2^31 by one multiply-high (Granlund & Montgomery 1994, theorem 4.2 with
// 31-bit dividends): with l = ceil(log2 d) and mul = ceil(2^(31 + l) / d), mul d = 2^(31 + l) + e with
// 0 <= e < d <= 2^l, so n mul / 2^(31 + l) = n / d + (n / 2^31) (e / 2^l) / d exceeds n / d by less than
// 1 / d and has its floor.  d > 2^(l - 1) keeps mul below 2^32 (d = 2^l gives 2^31).  The quotient is
// taken as the high word of (2 n) mul, shifted by l: 2 n fits 32 bits.
struct RayDiv {
  uint32_t mul;
  int shift;
};
inline RayDiv ray_div_of(int d) {
  int l = 0;
  while (((int64_t)1 << l) < d) ++l;
  const uint64_t p = (uint64_t)1 << (31 + l);
  return {(uint32_t)((p + (uint64_t)d - 1) / (uint64_t)d), l};
}
NERF_HD inline int ray_div(int n, uint32_t mul, int shift) {
  return (int)((uint32_t)(((uint64_t)((uint32_t)n << 1) * mul) >> 32) >> shift);
}

// 1 / s for s = 2^k, -127 < k < 127: the exponent field mirrored about the bias (the mantissa is
// zero), exact.
NERF_HD inline float pow2_recip(float s) {
  return __builtin_bit_cast(float, 0x7F000000u - __builtin_bit_cast(uint32_t, s));
}

}  // namespace nerf
