// Signed 8-bit digits of a scalar for the fixed-base tables (kernels_fixed.h): k = sum_w d_w 2^(8 w), d_w in [-128, 128].
// Included inside namespace cg1 by csrc/msm_gpu.hip (device + host) and by the host library (lazy_host.cpp, for the CPU tests):
// k_fixed_msm and the test hook cg1_fixed_digits are compiled from this one function.
//
// The recoding of k_generator_mul (kernels_generator.h), least significant window first: u = byte + carry; u > 128 becomes the digit
// u - 256 with a carry into the next window.  For k < r the top byte is at most 0x73 (r's top byte), 0x74 with the carry: the carry out
// of window 31 cannot occur, so 32 windows hold every canonical scalar.  A table base need not lie in G1, where d P depends on d itself
// and not only on d mod r: scalars >= r are REJECTED by the callers (fixed_scalar_below_r), never reduced.
#pragma once

constexpr int FIX_C = 8;                                   // window bits (== GEN_C: static_assert in kernels_fixed.h)
constexpr int FIX_HALF = 1 << (FIX_C - 1);                 // table entries per window: digits 1 .. 128
constexpr int FIX_WINDOWS = 256 / FIX_C;

// d[w * stride] = d_w.  Returns the carry out of the top window (0 for every scalar below r).
CG1_HD uint32_t fixed_digits(const uint32_t s[8], int16_t* d, int stride) {
  uint32_t carry = 0;
  for (int w = 0; w < FIX_WINDOWS; ++w) {
    const uint32_t v = (s[w >> 2] >> ((w & 3) * FIX_C)) & ((1u << FIX_C) - 1u);
    const uint32_t u = v + carry;
    carry = u > (uint32_t)FIX_HALF ? 1u : 0u;
    d[w * stride] = carry ? (int16_t)(-(int)((1u << FIX_C) - u)) : (int16_t)u;
  }
  return carry;
}

CG1_HD bool fixed_scalar_below_r(const uint32_t s[8]) {
  constexpr uint32_t R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
  for (int i = 7; i >= 0; --i) {
    if (s[i] != R[i]) return s[i] < R[i];
  }
  return false;
}
