// Exact relations in bulk: ok[i] = [ sum_j (+-) k_j P_j == identity ] for relations of at most CG1_EXACT_TERMS = 4 terms over a flat array
// of affine96 points and a flat array of 32-byte scalars -- the equalities the reference asserts directly for a proof that carries a point
// outside the prime-order subgroup (same_scalar.py:101-108: G_t z_t - cm_A.T_1 - alpha T_1, R z_k + H z_t - cm_A.T_2 - alpha T_2, ...;
// opening.py:73-76: s G + c k_G - A, s r_G + c k_r_G - B), where random weights are unsound.
// Part of the single translation unit csrc/msm_gpu.hip (included inside namespace cg1, after fp_row.h).
//
// One WAVE per relation, one limb per lane (fp_row.h).  The terms of a relation share ONE ladder (Straus): per 4-bit window four doublings
// of the accumulator, then for each term with a non-zero digit one addition of that term's table entry -- 252 doublings + at most 64 n_t
// additions for n_t scalar terms, where a ladder per term would pay the 252 doublings n_t times over.  The tables (15 multiples per term,
// built with 1 doubling + 13 additions) do not fit the register file beside each other (4 x 15 points x 4 coordinates = 240 VGPRs), so
// they live in LDS: 4 x 15 x 4 x 16 words = 15 360 B + 400 B of identity flags, records and scalars per wave, written by row 0 and read
// by every row (all four rows of a wave hold the same point).  That is ten waves per CU by LDS, 2.5 per SIMD, 2 560 relations in flight on the chip: the 4 x 1 024
// relations of a fully flagged batch of shuffle proofs take two rounds.  A term whose scalar is "one" has no table and no digits: its (signed) point is added once, after the ladder.
//
// Exact on all of E(Fp): no endomorphism split, no reduction of a scalar mod r (the scalar is its 256-bit integer), and every addition
// is row_add, whose branches -- an identity operand on either side, P + P, P - P -- are all live here: a base of small order has
// identities among its multiples (the flag travels with the table entry) and runs the accumulator through the identity; two terms over
// the same point meet acc == T and acc == -T.  The verdict is the accumulator's identity flag after the signed sum: no inversion, no
// compression.  Control flow depends on the scalars' digits (a zero digit adds nothing) and on the exceptional additions the operands
// force, never on a comparison with an expected value: there is no exit before the last term is added.
#pragma once

constexpr uint32_t EXACT_TERMS = 4, EXACT_NEG = 0x80000000u, EXACT_ONE = 0x7fffffffu, EXACT_NONE = 0xffffffffu;

// terms: n x EXACT_TERMS records {point index | EXACT_NONE (no term), scalar index | EXACT_ONE, with EXACT_NEG for a minus sign}.  The
// host layer has checked every index (capi_exact.h); a record out of range here costs its relation the verdict and reads nothing.
__global__ void __launch_bounds__(64) k_exact_relations(const uint32_t* __restrict__ points, uint32_t n_points, const uint32_t* __restrict__ scalars,
                                                        uint32_t n_scalars, const uint2* __restrict__ terms, uint32_t n, uint8_t* __restrict__ ok) {
  __shared__ uint32_t tab[EXACT_TERMS][15][4][16];
  __shared__ uint32_t tinf[EXACT_TERMS][15];
  __shared__ uint32_t rec[EXACT_TERMS][2], ssc[EXACT_TERMS][8];
  const uint32_t i = blockIdx.x;
  if (i >= n) return;
  const RowK k = row_constants();
  const uint32_t l = k.lane16;
  uint32_t r2 = 0;
#pragma unroll
  for (int t = 0; t < NL; ++t) r2 = l == (uint32_t)t ? fp_r2().l[t] : r2;
  auto load_point = [&](uint32_t idx, bool neg, xyzz_row& P) {                // 24 words x | y, standard form -> Montgomery rows, -P for a minus sign
    const uint32_t* w = points + 24ull * idx;
    uint32_t wd[24], any = 0;
    for (int t = 0; t < 24; ++t) { wd[t] = w[t]; any |= wd[t]; }
    P.X = row_mul(row_from_fp(fp_from_words(wd), l), r2, k);
    P.Y = row_mul(row_from_fp(fp_from_words(wd + 12), l), r2, k);
    if (neg) P.Y = row_norm_pass(row_norm_pass(k.kp3 - P.Y, l), l);
    P.ZZ = k.one; P.ZZZ = k.one; P.inf = any ? 0u : 1u;
  };

  // the relation's records and its scalars go through LDS, so that the loops below index them without unrolling (every read is wave-uniform)
  {
    const uint32_t lane = threadIdx.x & 63u;
    bool bad = false;
    if (lane < EXACT_TERMS) {
      const uint2 t = terms[(size_t)i * EXACT_TERMS + lane];
      const uint32_t si = t.y & ~EXACT_NEG;
      bad = t.x != EXACT_NONE && (t.x >= n_points || (si != EXACT_ONE && si >= n_scalars));
      rec[lane][0] = t.x; rec[lane][1] = t.y;
      const bool has_scalar = !bad && t.x != EXACT_NONE && si != EXACT_ONE;
      for (int w = 0; w < 8; ++w) ssc[lane][w] = has_scalar ? scalars[8ull * si + w] : 0u;
    }
    if (__ballot(bad)) { if (lane == 0) ok[i] = 0; return; }                  // (the whole wave; never taken behind the host layer)
  }
  __syncthreads();

  // the tables of the scalar terms: tab[j][d - 1] = d (+-P_j)
  uint32_t laddered = 0;                                                      // bit j: term j runs through the ladder
#pragma unroll 1
  for (uint32_t j = 0; j < EXACT_TERMS; ++j) {
    const uint32_t pj = rec[j][0], sj = rec[j][1];
    uint32_t any = 0;
    for (int w = 0; w < 8; ++w) any |= ssc[j][w];
    if (pj == EXACT_NONE || !any) continue;                                   // no term, a "one" term or a zero scalar: nothing in the ladder
    xyzz_row P1;
    load_point(pj, (sj & EXACT_NEG) != 0, P1);
    if (P1.inf) continue;                                                     // k * identity
    laddered |= 1u << j;
    xyzz_row cur = P1;
#pragma unroll 1
    for (uint32_t d = 0; d < 15; ++d) {
      if (d == 1) cur = row_dbl(P1, k);
      else if (d > 1) cur = row_add(cur, P1, k);
      if (k.row == 0) {
        tab[j][d][0][l] = cur.X; tab[j][d][1][l] = cur.Y; tab[j][d][2][l] = cur.ZZ; tab[j][d][3][l] = cur.ZZZ;
        if (l == 0) tinf[j][d] = cur.inf;                                     // (a multiple of a point of small order may be the identity)
      }
    }
  }
  __syncthreads();                                                            // one wave per block: orders row 0's stores before every row's loads

  xyzz_row acc; acc.X = acc.Y = acc.ZZ = acc.ZZZ = 0; acc.inf = 1;
  if (laddered) {
#pragma unroll 1
    for (int nib = 63; nib >= 0; --nib) {
      acc = row_dbl(row_dbl(row_dbl(row_dbl(acc, k), k), k), k);
#pragma unroll 1
      for (uint32_t j = 0; j < EXACT_TERMS; ++j) {
        const uint32_t d = (ssc[j][nib >> 3] >> ((nib & 7) * 4)) & 15u;       // wave-uniform
        if (d && ((laddered >> j) & 1u)) {
          xyzz_row Td;
          Td.X = tab[j][d - 1][0][l]; Td.Y = tab[j][d - 1][1][l]; Td.ZZ = tab[j][d - 1][2][l]; Td.ZZZ = tab[j][d - 1][3][l];
          Td.inf = tinf[j][d - 1];
          acc = row_add(acc, Td, k);
        }
      }
    }
  }
  // the "one" terms: +-P_j itself
#pragma unroll 1
  for (uint32_t j = 0; j < EXACT_TERMS; ++j) {
    const uint32_t pj = rec[j][0], sj = rec[j][1];
    if (pj == EXACT_NONE || (sj & ~EXACT_NEG) != EXACT_ONE) continue;
    xyzz_row A;
    load_point(pj, (sj & EXACT_NEG) != 0, A);
    acc = row_add(acc, A, k);
  }
  if ((threadIdx.x & 63u) == 0) ok[i] = acc.inf ? 1 : 0;
}

// dst block j (at j * dst_stride words) = src block idx[j] (at idx[j] * src_stride words), `words` words each, the words [clear_lo, clear_hi)
// of every copied block written as zero instead: the flagged subset of a batch compacted on the device -- its row-input blocks with the
// four same-scalar weights cleared, its own points -- for the second, weighted pass over that subset alone.  One block of 256 threads
// per destination block; idx has been checked on the host (capi_exact.h).
__global__ void __launch_bounds__(256) k_exact_gather(const uint32_t* __restrict__ src, size_t src_stride, const uint32_t* __restrict__ idx, uint32_t n_idx,
                                                      uint32_t* __restrict__ dst, size_t dst_stride, uint32_t words, uint32_t clear_lo, uint32_t clear_hi) {
  const uint32_t j = blockIdx.x;
  if (j >= n_idx) return;
  const uint32_t* s = src + (size_t)idx[j] * src_stride;
  uint32_t* d = dst + (size_t)j * dst_stride;
  for (uint32_t w = threadIdx.x; w < words; w += 256u) d[w] = (w >= clear_lo && w < clear_hi) ? 0u : s[w];
}
