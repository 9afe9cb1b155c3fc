// Signed c-bit digits of a scalar for the LIGHT tables (kernels_light.h), c = CG1_LIGHT_WINDOW_BITS < 8:
//     k = sum_w d_w 2^(c w),   d_w in [-2^(c-1), 2^(c-1)],   w = 0 .. LT_WINDOWS - 1.
// Included inside namespace cg1 by csrc/msm_gpu.hip (device + host) and by the host library (lazy_host.cpp, for the CPU tests):
// k_light_msm and the test hook cg1_light_digits are compiled from this one function.
//
// fixed_digits.h's recoding with a narrower window: u = window + carry; u > 2^(c-1) becomes the digit u - 2^c with a carry into the next
// window.  The windows cover ceil(256 / c) c bits >= 256, and a canonical scalar is below r < 2^255:
//   c = 4   64 windows; the top one holds 0x7 (r's top nibble) at most, 0x8 with the carry -- and 8 = 2^(c-1) stays a positive digit
//   c = 5   52 windows; window 50 may carry (bits 250 .. 254 of r are 11100b), window 51 holds bit 255 = 0 plus that carry
//   c = 3, 6, 7   86 / 43 / 37 windows cover 258 / 258 / 259 bits: the top window is 0 or 0x7 plus a carry, far below 2^(c-1)
// so the carry out of the top window cannot occur for any plan.  A table base need not lie in G1, where d P depends on d itself and not
// only on d mod r: scalars >= r are REJECTED by the callers (fixed_scalar_below_r), never reduced.
#pragma once

constexpr int LT_C = CG1_LIGHT_WINDOW_BITS;              // window bits
constexpr int LT_HALF = 1 << (LT_C - 1);                 // table entries per window: digits 1 .. 2^(c-1)
constexpr int LT_WINDOWS = (256 + LT_C - 1) / LT_C;
constexpr int LT_ENTRIES = LT_WINDOWS * LT_HALF;         // records per base
static_assert(LT_C >= 3 && LT_C < 8, "a light table is the one with windows narrower than the fixed tables' 8 bits");
static_assert(LT_WINDOWS == CG1_LIGHT_WINDOWS, "the header's window count is the recoding's");

// d[w * stride] = d_w.  Returns the carry out of the top window (0 for every scalar below r).
CG1_HD uint32_t light_digits(const uint32_t s[8], int8_t* d, int stride) {
  uint32_t carry = 0;
  for (int w = 0; w < LT_WINDOWS; ++w) {
    const int bit = w * LT_C, word = bit >> 5, sh = bit & 31;
    uint32_t v = s[word] >> sh;
    if (sh + LT_C > 32 && word + 1 < 8) v |= s[word + 1] << (32 - sh);      // a window that straddles two words (c = 3, 5, 6, 7)
    v &= (1u << LT_C) - 1u;
    const uint32_t u = v + carry;
    carry = u > (uint32_t)LT_HALF ? 1u : 0u;
    d[w * stride] = carry ? (int8_t)(-(int)((1u << LT_C) - u)) : (int8_t)u;
  }
  return carry;
}
