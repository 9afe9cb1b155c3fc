// The Fr half of the same-MSM argument's prover (same_msm.py:73-143) with the bases held FIXED: the scalar schedule of every MSM launch
// and the folds between two launches.  One source for the device (kernels_same_msm.h: one lane per term) and the host (lazy_host.cpp:
// cg1_same_msm_round_emulate, for the CPU tests) -- the way ipa_rounds.h is shared.
//
// The reference folds all three base vectors with gamma every round (same_msm.py:122-126).  Here a prover keeps ONE coefficient k[j] per
// ORIGINAL index j -- the product of the challenges of the rounds in which j sat in the right half (prover_kernels.same_msm_rounds_many)
// -- and a round's MSM over a folded half is an MSM over n0 / 2 unfolded bases with the coefficients multiplied into the scalars.
// With the current length 2 * half, lane t = b * half + i (b: which block of 2 * half original indices, i < half) owns
//     jl = b * 2 half + i  (the left half)        jr = jl + half  (the right half)
// and emits one term of each of the round's six MSMs, in the order the transcript absorbs their results:
//     L_A  base G[jr]   L_T  base T[jr]   L_U  base U[jr]     scalar x[i] k[jr]
//     R_A  base G[jl]   R_T  base T[jl]   R_U  base U[jl]     scalar x[half + i] k[jl]
// The G bases are records of a cg1_fixed table (the CRS), T and U records of a light table (kernels_light.h): two MSM launches per step,
// so two term arrays.  A prover's terms are contiguous in each, with h = n0 / 2:
//     the A array  [L_A: h][R_A: h]                  indices into the fixed table (the caller's g_index)
//     the TU array [L_T: h][L_U: h][R_T: h][R_U: h]  indices into the light table: T[j] at tu + j, U[j] at tu + n0 + j
// and for the step before the rounds, B_a = MSM(G, r) | B_t = MSM(T, r), B_u = MSM(U, r):  [B_a: n0]  and  [B_t: n0][B_u: n0].
#pragma once
#include "chain_rounds.h"

namespace cg1smsm {
using cg1fr::fr;
using cg1chain::load_le;
using cg1chain::put_term;

struct View {                                // one prover's state (Montgomery form) and its table indices
  fr* x;                                     // the current vector: positions [0, len)
  fr* k;                                     // per original index, n0
  const uint32_t* gi;                        // fixed-table indices of crs_G_vec, n0
  uint32_t tu;                               // light-table index of this prover's T[0]
  uint32_t n0;
};

// terms per prover and launch: step B and a round have the same counts (n0 = 2 h over G; 2 n0 = 4 h over T | U)
CG1FR_HD uint32_t a_terms(uint32_t n0) { return n0; }
CG1FR_HD uint32_t tu_terms(uint32_t n0) { return 2u * n0; }

// step B, lane j < n0 (same_msm.py:75-77)
CG1FR_HD void begin_term(const View& v, uint32_t j, const fr& r, uint32_t* tba, uint64_t* sca, uint32_t* tbl, uint64_t* scl) {
  put_term(tba, sca, j, v.gi[j], r);
  put_term(tbl, scl, j, v.tu + j, r);
  put_term(tbl, scl, v.n0 + j, v.tu + v.n0 + j, r);
}
// same_msm.py:90-91, lane j < n0
CG1FR_HD void blind_elem(const View& v, uint32_t j, const fr& alpha, const fr& r) { v.x[j] = cg1fr::fr_add(r, cg1fr::fr_mul(alpha, v.x[j])); }
// a round's terms, lane t < n0 / 2 (same_msm.py:101-106)
CG1FR_HD void round_term(const View& v, uint32_t half, uint32_t t, uint32_t* tba, uint64_t* sca, uint32_t* tbl, uint64_t* scl) {
  const uint32_t h = v.n0 / 2u, b = t / half, i = t - b * half, jl = b * 2u * half + i, jr = jl + half;
  const fr sl = cg1fr::fr_mul(v.x[i], v.k[jr]), sr = cg1fr::fr_mul(v.x[half + i], v.k[jl]);
  put_term(tba, sca, t, v.gi[jr], sl);
  put_term(tba, sca, h + t, v.gi[jl], sr);
  put_term(tbl, scl, t, v.tu + jr, sl);
  put_term(tbl, scl, h + t, v.tu + v.n0 + jr, sl);
  put_term(tbl, scl, 2u * h + t, v.tu + jl, sr);
  put_term(tbl, scl, 3u * h + t, v.tu + v.n0 + jl, sr);
}
// same_msm.py:122-126 with the bases left alone, lane t < n0 / 2: positions [0, half) of x are the folded vector afterwards.
// In place: lane t reads positions i and half + i and writes position i only.
CG1FR_HD void fold_elem(const View& v, uint32_t half, uint32_t t, const fr& gamma, const fr& gamma_inv) {
  const uint32_t b = t / half, i = t - b * half, jr = b * 2u * half + half + i;
  v.k[jr] = cg1fr::fr_mul(v.k[jr], gamma);
  if (b == 0u) v.x[i] = cg1fr::fr_add(v.x[i], cg1fr::fr_mul(gamma_inv, v.x[half + i]));
}

}  // namespace cg1smsm
