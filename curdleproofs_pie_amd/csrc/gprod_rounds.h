// The Fr half of the grand-product argument's prover (grand_prod.py:29-119) up to the hand-over to the inner-product argument, with the
// bases held FIXED: the element formulas, the completion of the IPA's blinders (ipa.py:27-48) and the term schedule of its two MSM
// launches.  One source for the device (kernels_gprod.h) and the host (lazy_host.cpp: cg1_gprod_emulate, for the CPU tests), like
// ipa_rounds.h, whose state (c, d, kG, kGp) and step-1 terms this header fills.
//
// n = ell + n_blinders; vec_G = crs_G_vec | crs_H_vec are n table bases gi[0 .. n) that never move.
//   launch 1   B' = MSM(vec_G, b | b_blinders)   what B must be for the reference's assertions (grand_prod.py:103-105) to hold
//              C  = MSM(vec_G, c | c_blinders)   c = the prefix products 1, b_0, b_0 b_1, ...  (:49-54)
//   launch 2   D  = MSM(vec_G, d[j] kGp[j])      the reference's own assertion :105 read as a definition: d_j = b_j beta^(j+1) - beta^j,
//                                                kGp[j] = beta^-(j+1) (:64-85), so the scalar is b_j - beta^-1; a blinder's is r_b + alpha
//              B_c = MSM(vec_G, r), B_d = MSM(vec_G, z[j] kGp[j])   ipa_rounds.h step1_term, over r and the COMPLETED z
// A prover's terms are contiguous: [B': n][C: n], then [D: n][B_c: n][B_d: n].
#pragma once
#include "ipa_rounds.h"

namespace cg1gprod {
using cg1fr::fr;
using cg1chain::load_le;
using cg1chain::put_term;

// bits of the chain's status word, above k_table_msm's (FX_BAD_*): CG1_GPROD_* of include/curdle_g1.h
constexpr uint32_t ST_BAD_COMMITMENT = 0x100u, ST_BAD_PRODUCT = 0x200u, ST_ZERO_BETA = 0x400u, ST_ZERO_C = 0x800u, ST_ZERO_DENOMINATOR = 0x1000u;
constexpr uint32_t ST_ALL = 0x1f00u;

CG1FR_HD uint32_t begin_terms(uint32_t n) { return 2u * n; }
CG1FR_HD uint32_t step_terms(uint32_t n) { return 3u * n; }
// term offsets of a prover whose first term is `first`: 3 values for launch 1, 4 for launch 2
CG1FR_HD void begin_offsets(uint32_t n, uint32_t first, uint32_t* o) { o[0] = first; o[1] = first + n; o[2] = first + 2u * n; }
CG1FR_HD void step_offsets(uint32_t n, uint32_t first, uint32_t* o) { o[0] = first; o[1] = first + n; o[2] = first + 2u * n; o[3] = first + 3u * n; }

// launch 1, lane j < n: b = b_j or a b blinder, c = the prefix product or a c blinder
CG1FR_HD void begin_term(const uint32_t* gi, uint32_t n, uint32_t j, const fr& b, const fr& c, uint32_t* tb, uint64_t* sc) {
  put_term(tb, sc, j, gi[j], b);
  put_term(tb, sc, n + j, gi[j], c);
}
// grand_prod.py:73-85, j < ell: d_j = b_j beta^(j+1) - beta^j, from beta^j
CG1FR_HD fr d_elem(const fr& b, const fr& beta, const fr& beta_pow_j) { return cg1fr::fr_mul(beta_pow_j, cg1fr::fr_sub(cg1fr::fr_mul(b, beta), cg1fr::fr_one())); }
// :87, a blinder: beta^(ell+1) (r_b + alpha)
CG1FR_HD fr d_blinder(const fr& rb_alpha, const fr& beta_ell1) { return cg1fr::fr_mul(beta_ell1, rb_alpha); }
// :95
CG1FR_HD fr inner_prod(const fr& r_p, const fr& gprod_result, const fr& beta_ell, const fr& beta_ell1) {
  return cg1fr::fr_sub(cg1fr::fr_add(cg1fr::fr_mul(r_p, beta_ell1), cg1fr::fr_mul(gprod_result, beta_ell)), cg1fr::fr_one());
}
// launch 2, lane j < n, once v.kGp is filled: D's term (d_kgp = d_j kGp[j], see above) and the IPA's step-1 terms behind it
CG1FR_HD void step_term(const cg1ipa::View& v, uint32_t j, const fr& d_kgp, const fr& r, const fr& z, uint32_t* tb, uint64_t* sc) {
  put_term(tb, sc, j, v.gi[j], d_kgp);
  cg1ipa::step1_term(v, j, r, z, tb + v.n0, sc + 4u * v.n0);
}

// generate_ipa_blinders (ipa.py:33-41) after its draws, with ONE inversion.  omega = <r, d> + <z[:n-2], c[:n-2]>, delta = <r[:n-2], z[:n-2]>;
// r2 = r[n-2], r1 = r[n-1], c2 = c[n-2], c1 = c[n-1].  The reference's two denominators are c2 and r1 - r2 c1 / c2 = e / c2 with
// e = r1 c2 - r2 c1, so
//     last_z = (r2 omega - delta c2) / e          penultimate_z = -(last_z c1 + omega) / c2
// and with t = 1 / (e c2): 1 / e = t c2, 1 / c2 = t e.  The caller tests c2 and e for zero BEFORE it inverts.
CG1FR_HD fr blinder_denominator(const fr& r2, const fr& r1, const fr& c2, const fr& c1) { return cg1fr::fr_sub(cg1fr::fr_mul(r1, c2), cg1fr::fr_mul(r2, c1)); }
CG1FR_HD void blinder_finish(const fr& omega, const fr& delta, const fr& r2, const fr& c2, const fr& c1, const fr& e, const fr& t, fr& penultimate_z, fr& last_z) {
  const fr inv_e = cg1fr::fr_mul(t, c2), inv_c2 = cg1fr::fr_mul(t, e);
  last_z = cg1fr::fr_mul(cg1fr::fr_sub(cg1fr::fr_mul(r2, omega), cg1fr::fr_mul(delta, c2)), inv_e);
  penultimate_z = cg1fr::fr_neg(cg1fr::fr_mul(cg1fr::fr_add(cg1fr::fr_mul(last_z, c1), omega), inv_c2));
}

}  // namespace cg1gprod
