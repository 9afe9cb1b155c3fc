// Light tables: window multiples of VARIABLE bases, built on the device in two launches, and the light plan of k_table_msm -- no doubling at MSM time.
// Part of the single translation unit csrc/msm_gpu.hip (included inside namespace cg1, after kernels_fixed.h).
//
// A cg1_fixed table (kernels_fixed.h) costs 512 KiB and ~0.35 ms per base: right for the CRS, which lives as long as the process, and
// unaffordable for bases that live for ONE proof -- vec_T and vec_U of the same-MSM argument (curdleproofs.py:124-136: R k and S k), 2 n
// points that each enter lg n + 1 MSMs once the round challenges fold into the scalars.  A light table pays a base's doublings once per
// proof with narrow windows: c = LT_C bits (light_digits.h), for bases B_0 .. B_{m-1}
//     tab[(b * LT_WINDOWS + w) * LT_HALF + (d - 1)] = d * 2^(c w) * B_b        w = 0 .. LT_WINDOWS - 1,  d = 1 .. 2^(c-1)
// as full XYZZ records (PointSum: 256 B; c = 4: 64 x 8 records = 128 KiB per base).  XYZZ and not affine, so that the build needs no
// inversion; the limbs are what row_store_sum leaves (nearly normal), and only row code reads them back.  Every record carries its own
// infinity flag: an all-zero base is the identity and so are all its entries, and a base of small order has identities among its
// multiples (the order-3 point (0, 2): 3 B = O).
//
// Build (exact for EVERY point of the curve: row_dbl is complete -- the curve has no point of order 2 -- and row_add takes the exact
// one-lane formulas for equal and opposite operands):
//   k_light_chain       one wave per base walks B, 2^c B, 2^(2c) B, ...: c (LT_WINDOWS - 1) dependent doublings, 252 at c = 4 -- the
//                       latency of the build (1.25 us each measured for this kernel: 315 us / 252, profiles/r08_light_table_kernels.txt)
//   k_light_multiples   one wave per (base, window): Q = 2^(c w) B is there; 2 Q = dbl(Q), 3 Q = 2 Q + Q, 4 Q = dbl(2 Q), ... one
//                       operation per record, the earlier multiples kept by the wave in row form (five words per lane and point).  The
//                       row arithmetic itself spills: the record shows 716 B of scratch here and 780 B in k_table_msm<LightPlan>
// One wave per RECORD, each walking its own double-and-add from Q (depth 3 to 4 at c = 4), would shorten the second chain from 7 steps
// to 4 at 22 operations per window instead of 7 -- and already one proof's table (256 bases x 64 windows = 16 384 waves, sixteen per
// SIMD) fills the chip, where the number of operations is what is paid: not built.
//
// The MSM over these records is k_table_msm (kernels_fixed.h) with LightPlan, below: the one kernel body -- grid, digits in LDS, one
// row_add per non-zero digit, the LDS tree, the ticketed slice join, the exports, the status bits -- and k_fixed_finish after it.
#pragma once

__device__ __forceinline__ size_t light_record(uint32_t b, uint32_t w, uint32_t mag) {      // index of |d| = mag, window w, base b
  return ((size_t)b * LT_WINDOWS + w) * LT_HALF + (mag - 1u);
}

// bases: n affine96 records (standard form; all-zero = the identity), already checked to be curve points.  Grid = n, one wave each.
__global__ void __launch_bounds__(64) k_light_chain(const uint32_t* __restrict__ bases96, uint32_t n, PointSum* __restrict__ tab) {
  const uint32_t b = blockIdx.x;
  if (b >= n) return;
  const RowK k = row_constants();
  const uint32_t l = k.lane16;
  uint32_t r2 = 0;
#pragma unroll
  for (int t = 0; t < NL; ++t) r2 = l == (uint32_t)t ? fp_r2().l[t] : r2;
  uint32_t wd[24], any = 0;
  for (int t = 0; t < 24; ++t) { wd[t] = bases96[24ull * b + t]; any |= wd[t]; }
  xyzz_row q;
  q.X = row_mul(row_from_fp(fp_from_words(wd), l), r2, k);
  q.Y = row_mul(row_from_fp(fp_from_words(wd + 12), l), r2, k);
  q.ZZ = k.one; q.ZZZ = k.one; q.inf = any ? 0u : 1u;
  if (q.inf) q.X = q.Y = q.ZZ = q.ZZZ = 0;
#pragma unroll 1
  for (uint32_t w = 0; w < (uint32_t)LT_WINDOWS; ++w) {
    if (w) {
#pragma unroll 1
      for (int i = 0; i < LT_C; ++i) q = row_dbl(q, k);
    }
    row_store_sum(tab + light_record(b, w, 1u), q, l);
  }
}

// Grid = n * LT_WINDOWS, one wave per (base, window): records d = 2 .. LT_HALF from record 1.
__global__ void __launch_bounds__(64) k_light_multiples(PointSum* __restrict__ tab, uint32_t n) {
  const uint32_t b = blockIdx.x / (uint32_t)LT_WINDOWS, w = blockIdx.x - b * (uint32_t)LT_WINDOWS;
  if (b >= n) return;
  const RowK k = row_constants();
  const uint32_t l = k.lane16;
  PointSum* rec = tab + light_record(b, w, 1u);
  xyzz_row T[LT_HALF];                                     // T[d - 1] = d Q
  T[0] = row_load_sum(rec, l);
#pragma unroll
  for (int d = 2; d <= LT_HALF; ++d) {
    T[d - 1] = (d & 1) ? fixed_add(T[d - 2], T[0], k) : row_dbl(T[d / 2 - 1], k);      // (d - 1) Q = +-Q only for a base of small order: exact
    row_store_sum(rec + (d - 1), T[d - 1], l);
  }
}

// The light plan: LT_WINDOWS signed c-bit digits per scalar (one byte each in LDS: the slice's digits are 8 KiB at c = 4, as the fixed
// plan's), full XYZZ records with their own infinity flags.
struct LightPlan {
  using Record = PointSum;
  using Digit = int8_t;
  static constexpr int WINDOWS = LT_WINDOWS;
  static __device__ __forceinline__ void digits(const uint32_t s[8], Digit* dst, int stride) { (void)light_digits(s, dst, stride); }
  static __device__ __forceinline__ xyzz_row load(const Record* tab, uint32_t base, uint32_t window, uint32_t magnitude, const RowK& k) {
    return row_load_sum(tab + light_record(base, window, magnitude), k.lane16);
  }
};
