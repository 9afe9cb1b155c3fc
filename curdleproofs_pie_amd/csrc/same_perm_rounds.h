// The Fr half of the same-permutation argument's wrapper (same_perm.py:27-72) around the grand-product argument, with the bases held
// FIXED: the polynomial factors, their blinders and the term schedule of the chain's first MSM launch.  One source for the device
// (kernels_same_perm.h) and the host (lazy_host.cpp: cg1_same_perm_emulate, for the CPU tests), like gprod_rounds.h, whose launch 1 this
// header widens from two MSMs per prover to four.
//
// n = ell + n_blinders; vec_G = crs_G_vec | crs_H_vec are n table bases gi[0 .. n) that never move.  With alpha, beta drawn:
//   b_i = vec_a[perm[i]] + perm[i] alpha + beta   (i < ell, :48-51)        b_blinder_k = vec_a_blinders[k] + alpha vec_m_blinders[k]   (:57-59)
//   launch 1   A' = MSM(vec_G, vec_a o perm | vec_a_blinders)   what A must be, and
//              M' = MSM(vec_G, perm | vec_m_blinders)           what M must be, for
//              B' = MSM(vec_G, b | b_blinders)                  to be the reference's B = A + alpha M + beta sum G_i (:55)
//              C  = MSM(vec_G, c | c_blinders)                  gprod_rounds.h
// B = B' exactly when A - A' + alpha (M - M') = O, which is also exactly when the reference's assertion grand_prod.py:105 holds.  The
// chain asks for A = A' and M = M' (two 48-byte comparisons): stricter only on the event A - A' = -alpha (M - M') != O, and alpha is
// drawn after A and M are absorbed, so a prover meets that event with negligible probability.
// A prover's terms are contiguous: [A': n][M': n][B': n][C: n].
#pragma once
#include "gprod_rounds.h"

namespace cg1sperm {
using cg1fr::fr;
using cg1chain::load_le;
using cg1chain::put_term;

// bits of the chain's status word, above the grand-product argument's (cg1gprod::ST_*): CG1_SAME_PERM_* of include/curdle_g1.h
constexpr uint32_t ST_BAD_A = 0x2000u, ST_BAD_M = 0x4000u;

CG1FR_HD uint32_t begin_terms(uint32_t n) { return 4u * n; }
// term offsets of a prover whose first term is `first`: 5 values
CG1FR_HD void begin_offsets(uint32_t n, uint32_t first, uint32_t* o) { for (uint32_t q = 0; q <= 4u; ++q) o[q] = first + q * n; }

// same_perm.py:49-51: m = perm[i] enters as the small scalar it is
CG1FR_HD fr factor(const fr& a_perm, uint32_t m, const fr& alpha, const fr& beta) {
  return cg1fr::fr_add(cg1fr::fr_add(a_perm, cg1fr::fr_mul(cg1fr::fr_from_u64(m), alpha)), beta);
}
// :57-59
CG1FR_HD fr blinder(const fr& a_blinder, const fr& m_blinder, const fr& alpha) { return cg1fr::fr_add(a_blinder, cg1fr::fr_mul(alpha, m_blinder)); }

// launch 1, lane j < n: a = vec_a[perm[j]] or an a blinder, m = perm[j] or an m blinder, b and c as in cg1gprod::begin_term, whose
// schedule the last two lists keep
CG1FR_HD void begin_term(const uint32_t* gi, uint32_t n, uint32_t j, const fr& a, const fr& m, const fr& b, const fr& c, uint32_t* tb, uint64_t* sc) {
  put_term(tb, sc, j, gi[j], a);
  put_term(tb, sc, n + j, gi[j], m);
  cg1gprod::begin_term(gi, n, j, b, c, tb + 2u * n, sc + 8u * n);
}

}  // namespace cg1sperm
