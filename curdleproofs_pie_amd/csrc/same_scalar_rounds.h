// The Fr half of the shuffle prover's same-scalar block (curdleproofs.py:92-116 with same_scalar.py:39-69): R, S, cm_T, cm_U and the whole
// of SameScalarProof.new with the bases held FIXED -- the term schedule of the block's one MSM launch and the three responses.  One source
// for the device (kernels_same_scalar.h: one lane per element) and the host (lazy_host.cpp: cg1_same_scalar_emulate, for the CPU tests),
// like same_msm_rounds.h.
//
// The reference multiplies R = MSM(vec_R, vec_a) by k and by r_k (and S likewise).  For bases of order r those products are MSMs over
// the same bases with the factor multiplied into the scalars, so every point the block emits is ONE MSM over vec_R | vec_S | G_t | G_u | H
// and no base is ever multiplied on its own.  The ten MSMs, in the order the transcript absorbs their results (same_scalar.py:46-62):
//     R        sum a_i R_i                       S        sum a_i S_i
//     T.T_1    r_t G_t                           T.T_2    sum (k a_i) R_i + r_t H
//     U.T_1    r_u G_u                           U.T_2    sum (k a_i) S_i + r_u H
//     A.T_1    r_a G_t                           A.T_2    sum (r_k a_i) R_i + r_a H
//     B.T_1    r_b G_u                           B.T_2    sum (r_k a_i) S_i + r_b H
// The bases are records of ONE light table (kernels_light.h) per call: G_t, G_u, H at 0, 1, 2, shared by all provers, then per prover
// vec_R | vec_S, R_j at rs + j and S_j at rs + ell + j.  A prover's 6 ell + 8 terms are contiguous, list after list.
#pragma once
#include "chain_rounds.h"

namespace cg1sscalar {
using cg1fr::fr;
using cg1chain::load_le;
using cg1chain::put_term;

// bit of the chain's status word, above the same-permutation argument's (cg1sperm::ST_*): CG1_SAME_SCALAR_NOT_G1 of include/curdle_g1.h
constexpr uint32_t ST_NOT_G1 = 0x8000u;

constexpr uint32_t MSMS = 10;                // per prover
constexpr uint32_t BASE_GT = 0, BASE_GU = 1, BASE_H = 2, SHARED_BASES = 3;

CG1FR_HD uint32_t terms(uint32_t ell) { return 6u * ell + 8u; }
// where list q of a prover begins among its terms; q = MSMS: their count
// (lengths ell, ell, then four commitments of 1 and ell + 1)
CG1FR_HD uint32_t list_begin(uint32_t ell, uint32_t q) { return q < 2u ? q * ell : 2u * ell + ((q - 2u) >> 1) * (ell + 2u) + ((q - 2u) & 1u); }
// term offsets of a prover whose first term is `first`: MSMS + 1 values
CG1FR_HD void offsets(uint32_t ell, uint32_t first, uint32_t* o) { for (uint32_t q = 0; q <= MSMS; ++q) o[q] = first + list_begin(ell, q); }

// element j < ell of vec_a: its six terms.  rs: the light-table index of this prover's R_0
CG1FR_HD void elem_terms(uint32_t ell, uint32_t rs, uint32_t j, const fr& a, const fr& k, const fr& r_k, uint32_t* tb, uint64_t* sc) {
  const fr ka = cg1fr::fr_mul(k, a), rka = cg1fr::fr_mul(r_k, a);
  const uint32_t R = rs + j, S = rs + ell + j;
  put_term(tb, sc, list_begin(ell, 0) + j, R, a);
  put_term(tb, sc, list_begin(ell, 1) + j, S, a);
  put_term(tb, sc, list_begin(ell, 3) + j, R, ka);
  put_term(tb, sc, list_begin(ell, 5) + j, S, ka);
  put_term(tb, sc, list_begin(ell, 7) + j, R, rka);
  put_term(tb, sc, list_begin(ell, 9) + j, S, rka);
}
// the eight terms over G_t, G_u, H (commitment.py:30); which < 4: the commitment T, U, A or B with its blinder r
CG1FR_HD void blinder_terms(uint32_t ell, uint32_t which, const fr& r, uint32_t* tb, uint64_t* sc) {
  put_term(tb, sc, list_begin(ell, 2u + 2u * which), (which & 1u) ? BASE_GU : BASE_GT, r);
  put_term(tb, sc, list_begin(ell, 3u + 2u * which) + ell, BASE_H, r);
}
// same_scalar.py:65-67; which: z_k (secret k, blinder r_k), z_t (r_t, r_a), z_u (r_u, r_b)
CG1FR_HD fr response(const fr& blinder, const fr& secret, const fr& alpha) { return cg1fr::fr_add(blinder, cg1fr::fr_mul(secret, alpha)); }

// The proof's 48-byte slot of encoding q of the transcript's order [R, S, T.T_1, T.T_2, U.T_1, U.T_2, A.T_1, A.T_2, B.T_1, B.T_2]:
// cm_T | cm_U | R | S | cm_A | cm_B, then z_k | z_t | z_u (CurdleProofsProof.to_bytes without M, A and the same-permutation proof)
CG1FR_HD uint32_t proof_slot(uint32_t q) { return q < 2u ? q + 4u : (q < 6u ? q - 2u : q); }
constexpr uint32_t PROOF_BYTES = MSMS * 48u + 3u * 32u;

}  // namespace cg1sscalar
