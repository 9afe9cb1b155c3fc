// Which trackers does a set of Whisk secrets open?  bit (i, j) = [k_j * r_G_i == k_r_G_i] for T trackers and V secrets (util.py:35-36,
// the relation opening.py proves): V * T independent scalar multiplications of VARIABLE bases.
// Part of the single translation unit csrc/msm_gpu.hip (included inside namespace cg1, after kernels_light.h).
//
// A tracker's light table (kernels_light.h: the signed 4-bit window multiples d * 2^(4 w) * r_G, built once in two launches, exact for
// every point of the curve) serves every secret: a pair then costs at most LT_WINDOWS = 64 full XYZZ additions and NO doubling, where
// k_batch_mul pays 255 doublings and ~128 mixed additions per pair; and the verdict needs no inversion: with S = (x, y) affine from the
// decoder, k R == S  <=>  X == x ZZ and Y == y ZZZ.
//
//   k_tracker_normalise   the records of a tile, once after the build: the carries of the nearly-normal limbs row_store_sum leaves
//                         (<= 2^28 + 3, fp_row.h) are finished, so that every stored coordinate is in the N-limb form the one-lane
//                         formulas of g1_xyzz.h state their bounds for (limbs 0..12 < 2^28; the value is unchanged: X < 10.1 p from
//                         row_add, < 7.1 p from row_dbl, Y, ZZ, ZZZ < 2 p)
//   k_tracker_match       one LANE per pair; the 64 lanes of a wave hold 64 secrets against ONE tracker, so the eight records of a
//                         window are read by the whole wave through the cache.  Windows are added in ascending order w = 0 .. 63 with
//                         xyzz_add, which is exact for equal and opposite operands and for identity operands on either side (a base of
//                         small order has identities among its records and runs the accumulator through the identity); a negative
//                         digit negates the record's Y (3p - Y, carried: < 5 p in N-limb form), a zero digit adds nothing.  The wave's
//                         64 verdicts leave as ONE 64-bit word, written by lane 0 with an ordinary store: no atomics, every word of
//                         the bitmap written exactly once per call.
//
// A table is built once per tracker and pays off over many secrets.  For a handful of secrets the build's chain (252 dependent doublings per
// tile) and a tile's 64 dependent additions cost more than a plain ladder per pair, so the host layer sends such calls down
//   k_tracker_replicate   scalars[j * T + i] = k_j, on the device, from the V secrets
//   k_batch_mul           (kernels_batch.h) one double-and-add ladder per pair, exact for every curve point, affine96 out
//   k_tracker_compare     one thread per word of the bitmap: the canonical affine words of k_j R_i against the decoder's of S_i (the
//                         identity is the all-zero record on both sides), the same statuses
// with the same bits (measured crossover: DESIGN section 17).
//
// No subgroup test and no GLV split: nothing here folds scalars, a secret is refused unless it is below r (never reduced: for a base
// outside G1, d P depends on d itself), and the table is exact outside G1.
#pragma once

// nrec records x 4 coordinates, one thread each
__global__ void __launch_bounds__(256) k_tracker_normalise(PointSum* __restrict__ tab, uint32_t nrec) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x, rec = t >> 2, c = t & 3u;
  if (rec >= nrec) return;
  uint32_t* l = tab[rec].c[c];
  fp v;
#pragma unroll
  for (int i = 0; i < NL; ++i) v.l[i] = l[i];
  v = fp_norm(v);
#pragma unroll
  for (int i = 0; i < NL; ++i) l[i] = v.l[i];
}

// Grid = (ceil(nk / 64), nt), one wave per block: tracker i of the tile against secrets 64 x .. 64 x + 63.
//   tab      the tile's light table: nt x LT_ENTRIES normalised records of r_G
//   s_aff    the tile's k_r_G as the decoder left them (affine96 standard-form words, all-zero = the identity or a failed decode)
//   st_r, st_s   the decoder's status bytes of the tile's r_G and k_r_G (non-zero: the tracker's row is zero)
//   ks       nk x 8 words, little-endian; a secret >= r leaves a zero column
//   bitmap   row 0 of the tile, `words` 64-bit words per tracker (words = ceil(nk / 64) = gridDim.x)
__global__ void __launch_bounds__(64) k_tracker_match(const PointSum* __restrict__ tab, const uint32_t* __restrict__ s_aff, const uint8_t* __restrict__ st_r,
                                                      const uint8_t* __restrict__ st_s, const uint32_t* __restrict__ ks, uint32_t nk, uint32_t nt,
                                                      unsigned long long* __restrict__ bitmap, uint32_t words) {
  __shared__ int8_t s_dig[LT_WINDOWS][64];
  const uint32_t i = blockIdx.y, lane = threadIdx.x, j = blockIdx.x * 64u + lane;
  if (i >= nt || blockIdx.x >= words) return;                  // (the whole wave)
  unsigned long long* out = bitmap + (size_t)i * words + blockIdx.x;
  if (st_r[i] | st_s[i]) {                                     // (the whole wave)
    if (lane == 0) *out = 0ull;
    return;
  }
  uint32_t s[8];
  bool live = j < nk;
#pragma unroll
  for (int t = 0; t < 8; ++t) s[t] = live ? ks[8ull * j + t] : 0u;
  live = live && fixed_scalar_below_r(s);
  if (!live) {
#pragma unroll
    for (int t = 0; t < 8; ++t) s[t] = 0;
  }
  (void)light_digits(s, &s_dig[0][lane], 64);                  // each lane reads back only what it wrote: no barrier

  xyzz acc = xyzz_identity();
#pragma unroll 1
  for (uint32_t w = 0; w < (uint32_t)LT_WINDOWS; ++w) {
    const int d = s_dig[w][lane];
    if (d != 0) {
      xyzz b = load_sum(tab + light_record(i, w, (uint32_t)(d < 0 ? -d : d)));
      const fp ny = fp_norm(fp_neg<3>(b.Y));
#pragma unroll
      for (int t = 0; t < NL; ++t) b.Y.l[t] = d < 0 ? ny.l[t] : b.Y.l[t];
      acc = xyzz_add(acc, b);
    }
  }

  uint32_t sw[24], any = 0;
#pragma unroll
  for (int t = 0; t < 24; ++t) { sw[t] = s_aff[24ull * i + t]; any |= sw[t]; }
  bool match;
  if (!any) {
    match = acc.inf != 0;                                      // S is the identity
  } else if (acc.inf) {
    match = false;
  } else {
    const fp x = fp_to_mont(fp_from_words(sw)), y = fp_to_mont(fp_from_words(sw + 12));
    const fp P = fp_sub<12>(fp_mul(x, acc.ZZ), acc.X);         // value < 13.1 p (xyzz_madd's test for equal operands)
    const fp R = fp_sub<6>(fp_mul(y, acc.ZZZ), acc.Y);         // value < 7.1 p
    match = fp_is_zero_mod_p(P, 14) && fp_is_zero_mod_p(R, 8);
  }
  const unsigned long long word = __ballot(match && live);
  if (lane == 0) *out = word;
}

// ---- the ladder route for a handful of secrets
__global__ void __launch_bounds__(256) k_tracker_replicate(const uint32_t* __restrict__ ks, uint32_t nk, uint32_t nt, uint32_t* __restrict__ out) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nk * nt) return;
  const uint32_t j = p / nt;
#pragma unroll
  for (int t = 0; t < 8; ++t) out[8ull * p + t] = ks[8ull * j + t];
}

// prod: nk x nt affine96 records, record j * nt + i = k_j R_i (k_batch_mul).  One thread per word (i, wj) of the bitmap.
__global__ void __launch_bounds__(256) k_tracker_compare(const uint32_t* __restrict__ prod, const uint32_t* __restrict__ s_aff, const uint8_t* __restrict__ st_r,
                                                         const uint8_t* __restrict__ st_s, const uint32_t* __restrict__ ks, uint32_t nk, uint32_t nt,
                                                         unsigned long long* __restrict__ bitmap, uint32_t words) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x, i = t / words, wj = t - i * words;
  if (i >= nt) return;
  unsigned long long bits = 0;
  if (!(st_r[i] | st_s[i])) {
    uint32_t sw[24];
#pragma unroll
    for (int c = 0; c < 24; ++c) sw[c] = s_aff[24ull * i + c];
    const uint32_t hi = min(nk, 64u * wj + 64u);
    for (uint32_t j = 64u * wj; j < hi; ++j) {
      uint32_t s[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) s[c] = ks[8ull * j + c];
      const uint32_t* q = prod + 24ull * ((size_t)j * nt + i);
      uint32_t diff = 0;
#pragma unroll
      for (int c = 0; c < 24; ++c) diff |= q[c] ^ sw[c];
      if (diff == 0 && fixed_scalar_below_r(s)) bits |= 1ull << (j & 63u);
    }
  }
  bitmap[(size_t)i * words + wj] = bits;
}
