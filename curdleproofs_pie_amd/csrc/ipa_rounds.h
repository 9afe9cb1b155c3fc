// The Fr half of the inner-product argument's prover (ipa.py:97-151) with the bases held FIXED: the scalar schedule of every MSM launch
// and the folds between two launches.  One source for the device (kernels_ipa.h: one lane per term) and the host (lazy_host.cpp:
// cg1_ipa_round_emulate, for the CPU tests) -- the way fixed_digits.h is shared.
//
// The reference folds the bases every round (G = G_L + gamma G_R).  Here a prover keeps, per ORIGINAL index j, the product kG[j] /
// kGp[j] of the challenges of the rounds in which j sat in the right half (prover_kernels.ipa_rounds_many has the derivation), and a
// round's MSM over a folded half becomes an MSM over n0 / 2 table bases with the coefficients multiplied into the scalars.  With the
// current length 2 * half, lane t = b * half + i (b: which block of 2 * half original indices, i < half) owns
//     jl = b * 2 half + i  (current position i, the left half)        jr = jl + half  (current position half + i, the right half)
// and emits one term of each of the round's four MSMs, in the order the transcript absorbs their results:
//     L_C  base G[jr]   scalar c[i]        kG[jr]        (+ the term  H  <c_L, d_R> kH  at the end)
//     L_D  base G'[jl]  scalar d[half + i] kGp[jl]
//     R_C  base G[jl]   scalar c[half + i] kG[jl]        (+ the term  H  <c_R, d_L> kH)
//     R_D  base G'[jr]  scalar d[i]        kGp[jr]
// kGp starts at the caller's G' coefficients (grand_prod.py:64-71 as scalars) or 1; kH is beta: crs_H * beta is never a point.
// A prover's terms are contiguous: [L_C: h + 1][L_D: h][R_C: h + 1][R_D: h] with h = n0 / 2, every round.
#pragma once
#include "chain_rounds.h"

namespace cg1ipa {
using cg1fr::fr;
using cg1chain::load_le;
using cg1chain::put_term;

struct View {                                // one prover's state (Montgomery form) and its table indices
  fr* c; fr* d;                              // the current vectors: positions [0, len)
  fr* kG; fr* kGp;                           // per original index, n0 each
  const uint32_t* gi; const uint32_t* gpi;   // table indices of crs_G_vec / crs_G_prime_vec, n0 each
  uint32_t hi;                               // table index of crs_H
  uint32_t n0;
};

CG1FR_HD uint32_t round_terms(uint32_t n0) { return 2u * n0 + 2u; }
CG1FR_HD uint32_t step1_terms(uint32_t n0) { return 2u * n0; }
// term offsets of a prover whose first term is `first`: 5 values for a round, 3 for step 1 (B_c over G, B_d over G')
CG1FR_HD void round_offsets(uint32_t n0, uint32_t first, uint32_t* o) {
  const uint32_t h = n0 / 2u;
  o[0] = first; o[1] = o[0] + h + 1u; o[2] = o[1] + h; o[3] = o[2] + h + 1u; o[4] = o[3] + h;
}
CG1FR_HD void step1_offsets(uint32_t n0, uint32_t first, uint32_t* o) { o[0] = first; o[1] = first + n0; o[2] = first + 2u * n0; }

// step 1, lane j < n0:  B_c = MSM(G, r_c),  B_d = MSM(G', r_d)  (ipa.py:97-98)
CG1FR_HD void step1_term(const View& v, uint32_t j, const fr& rc, const fr& rd, uint32_t* tb, uint64_t* sc) {
  put_term(tb, sc, j, v.gi[j], rc);
  put_term(tb, sc, v.n0 + j, v.gpi[j], cg1fr::fr_mul(rd, v.kGp[j]));
}
// ipa.py:107-109, lane j < n0
CG1FR_HD void blind_elem(const View& v, uint32_t j, const fr& alpha, const fr& rc, const fr& rd) {
  v.c[j] = cg1fr::fr_add(rc, cg1fr::fr_mul(alpha, v.c[j]));
  v.d[j] = cg1fr::fr_add(rd, cg1fr::fr_mul(alpha, v.d[j]));
}
// a round's terms, lane t < n0 / 2 (ipa.py:126-129).  pl / pr: this lane's share of <c_L, d_R> / <c_R, d_L> (zero outside block 0)
CG1FR_HD void round_term(const View& v, uint32_t half, uint32_t t, uint32_t* tb, uint64_t* sc, fr& pl, fr& pr) {
  const uint32_t h = v.n0 / 2u, b = t / half, i = t - b * half, jl = b * 2u * half + i, jr = jl + half;
  const fr cl = v.c[i], cr = v.c[half + i], dl = v.d[i], dr = v.d[half + i];
  put_term(tb, sc, t, v.gi[jr], cg1fr::fr_mul(cl, v.kG[jr]));
  put_term(tb, sc, h + 1u + t, v.gpi[jl], cg1fr::fr_mul(dr, v.kGp[jl]));
  put_term(tb, sc, 2u * h + 1u + t, v.gi[jl], cg1fr::fr_mul(cr, v.kG[jl]));
  put_term(tb, sc, 3u * h + 2u + t, v.gpi[jr], cg1fr::fr_mul(dl, v.kGp[jr]));
  if (b == 0u) { pl = cg1fr::fr_mul(cl, dr); pr = cg1fr::fr_mul(cr, dl); }
  else { pl = cg1fr::fr_zero(); pr = cg1fr::fr_zero(); }
}
// the two H terms, once the inner products are summed
CG1FR_HD void round_h_terms(const View& v, const fr& kH, const fr& ip_l, const fr& ip_r, uint32_t* tb, uint64_t* sc) {
  const uint32_t h = v.n0 / 2u;
  put_term(tb, sc, h, v.hi, cg1fr::fr_mul(ip_l, kH));
  put_term(tb, sc, 3u * h + 1u, v.hi, cg1fr::fr_mul(ip_r, kH));
}
// ipa.py:142-146 with the bases left alone, lane t < n0 / 2: positions [0, half) of c and d are the folded vectors afterwards.
// In place: lane t reads positions i and half + i and writes position i only.
CG1FR_HD void fold_elem(const View& v, uint32_t half, uint32_t t, const fr& gamma, const fr& gamma_inv) {
  const uint32_t b = t / half, i = t - b * half, jr = b * 2u * half + half + i;
  v.kG[jr] = cg1fr::fr_mul(v.kG[jr], gamma);
  v.kGp[jr] = cg1fr::fr_mul(v.kGp[jr], gamma_inv);
  if (b == 0u) {
    v.c[i] = cg1fr::fr_add(v.c[i], cg1fr::fr_mul(gamma_inv, v.c[half + i]));
    v.d[i] = cg1fr::fr_add(v.d[i], cg1fr::fr_mul(gamma, v.d[half + i]));
  }
}

}  // namespace cg1ipa
