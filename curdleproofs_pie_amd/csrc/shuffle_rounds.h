// The Fr half of the head of a whole shuffle proof (curdleproofs.py:71-78, :92-93, :118-138) with the bases held FIXED: everything
// CurdleProofsProof.new forms from curdleproofs_vec_a, the permutation and the caller's draws BEFORE any of its three arguments has a
// challenge -- the term schedule of A and A', vec_x of the same-MSM argument, and (taken from same_scalar_rounds.h, not copied) the terms
// of the same-scalar block's ten MSMs.  One source for the device (kernels_shuffle.h: one lane per element) and the host (lazy_host.cpp:
// cg1_shuffle_begin_emulate, for the CPU tests), like the other *_rounds.h.
//
// n = ell + N_BLINDERS, N_BLINDERS = 4.  With vec_x = vec_a o perm | vec_a_blinders (2) | r_t | r_u (curdleproofs.py:138):
//     A   = MSM(vec_G | vec_H,                   vec_a o perm | vec_a_blinders | 0 | 0)       (:77)
//     A'  = MSM(vec_G | vec_H[:2] | G_t | G_u,   vec_x)                                       = A + cm_T.T_1 + cm_U.T_1  (:118)
// because T_1 = r G_t (commitment.py:30): A' is an MSM over table bases like A, needs no point addition and no result of the
// same-scalar block.  A prover's 2 n terms are contiguous: [A: n][A': n].
#pragma once
#include "same_scalar_rounds.h"

namespace cg1shuffle {
using cg1fr::fr;
using cg1chain::load_le;
using cg1chain::put_term;

constexpr uint32_t N_BLINDERS = 4;           // curdleproofs.py:24
constexpr uint32_t HEAD_MSMS = 2;            // per prover: A, A'

CG1FR_HD uint32_t head_terms(uint32_t n) { return HEAD_MSMS * n; }
// term offsets of a prover whose first term is `first`: 3 values
CG1FR_HD void head_offsets(uint32_t n, uint32_t first, uint32_t* o) { for (uint32_t q = 0; q <= HEAD_MSMS; ++q) o[q] = first + q * n; }

// get_permutation (util.py:93-96) reads vec_a[perm[j]]; the entry has refused perm[j] >= ell, and the gather stays in range regardless
CG1FR_HD uint32_t gather_index(uint32_t ell, uint32_t m) { return m < ell ? m : ell - 1u; }

// element j < n of vec_x.  va: vec_a (ell canonical scalars), abl: vec_a_blinders (2 canonical scalars)
CG1FR_HD fr x_elem(uint32_t ell, uint32_t j, const uint64_t* va, const uint32_t* perm, const uint64_t* abl, const fr& r_t, const fr& r_u) {
  if (j < ell) return load_le(va + 4u * gather_index(ell, perm[j]));
  if (j < ell + 2u) return load_le(abl + 4u * (j - ell));
  return j == ell + 2u ? r_t : r_u;
}
// lane j < n: its term of A (over gi_a = vec_G | vec_H; the last two scalars are zero) and of A' (over gi_m = vec_G | vec_H[:2] | G_t |
// G_u), and vec_x[j] as the same-MSM chain reads it (canonical, 4 words)
CG1FR_HD void head_term(const uint32_t* gi_a, const uint32_t* gi_m, uint32_t n, uint32_t ell, uint32_t j, const fr& x, uint32_t* tb, uint64_t* sc, uint64_t* vx) {
  put_term(tb, sc, j, gi_a[j], j < ell + 2u ? x : cg1fr::fr_zero());
  put_term(tb, sc, n + j, gi_m[j], x);
  cg1fr::fr_to_le32(x, reinterpret_cast<uint8_t*>(vx + 4u * j));
}

}  // namespace cg1shuffle
