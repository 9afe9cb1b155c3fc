// k_shuffle_begin: the first kernel of a whole shuffle proof proved on the device (capi_shuffle.h) -- the terms of every MSM of
// CurdleProofsProof.new that does not depend on a transcript challenge later than curdleproofs_vec_a:
//     A | A'            two MSMs of n terms over the CRS table (k_table_msm<FixedPlan>), shuffle_rounds.h
//     vec_x             a o perm | a_blinders | r_t | r_u, written where the same-MSM chain's begin phase reads it (SmsmArgs::vx)
//     the ten MSMs      of the same-scalar block (k_table_msm<LightPlan>): what k_sscalar_step's begin phase writes, from the same
//                       functions of same_scalar_rounds.h
// Part of the single translation unit csrc/msm_gpu.hip (after kernels_same_scalar.h).
//
// One workgroup per prover, 256 threads, lane t owns elements t, t + 256, ... -- the begin phase of the step skeleton (kernels_chain.h)
// without its transcript block: no LDS, no inversion, no transcript, no trap.  The host has refused perm[i] >= ell before the launch, and
// the gather clamps all the same (shuffle_rounds.h: gather_index).
#pragma once
#include "shuffle_rounds.h"
#include "kernels_same_scalar.h"

namespace cg1shuffle {

constexpr uint32_t SH_THREADS = 256;

struct ShuffleBeginArgs {
  uint32_t ell;
  const uint64_t* va;                        // [P][ell] canonical: curdleproofs_vec_a
  const uint32_t* perm;                      // [P][ell], every entry < ell
  const uint64_t* k;                         // [P] canonical
  const uint64_t* bl;                        // [P][5] canonical: r_t r_u r_a r_b r_k
  const uint64_t* abl;                       // [P][2] canonical: vec_a_blinders
  const uint32_t* gi_a;                      // [P][n]: table indices of vec_G | vec_H
  const uint32_t* gi_m;                      // [P][n]: table indices of vec_G | vec_H[:2] | G_t | G_u
  uint32_t* tb; uint64_t* sc;                // the term arrays of A | A': [P][2 n]
  uint64_t* vx;                              // [P][n] canonical: vec_x
  uint32_t* ss_tb; uint64_t* ss_sc;          // the same-scalar block's term arrays: [P][6 ell + 8]
};

__global__ void __launch_bounds__(SH_THREADS) k_shuffle_begin(ShuffleBeginArgs a) {
  const uint32_t tid = threadIdx.x, p = blockIdx.x, ell = a.ell, n = ell + N_BLINDERS;
  const uint64_t* va = a.va + 4u * (size_t)p * ell;
  const uint32_t* perm = a.perm + (size_t)p * ell;
  const uint64_t* bl = a.bl + 20u * (size_t)p;
  const uint64_t* abl = a.abl + 8u * (size_t)p;
  const uint32_t* gi_a = a.gi_a + (size_t)p * n;
  const uint32_t* gi_m = a.gi_m + (size_t)p * n;
  uint32_t* tb = a.tb + (size_t)p * head_terms(n);
  uint64_t* sc = a.sc + 4u * (size_t)p * head_terms(n);
  uint64_t* vx = a.vx + 4u * (size_t)p * n;
  const fr r_t = load_le(bl), r_u = load_le(bl + 4u);

  // ---- A, A' and vec_x
  for (uint32_t j = tid; j < n; j += SH_THREADS) head_term(gi_a, gi_m, n, ell, j, x_elem(ell, j, va, perm, abl, r_t, r_u), tb, sc, vx);

  // ---- the same-scalar block's begin phase (k_sscalar_step, SS_BEGIN)
  uint32_t* ss_tb = a.ss_tb + (size_t)p * cg1sscalar::terms(ell);
  uint64_t* ss_sc = a.ss_sc + 4u * (size_t)p * cg1sscalar::terms(ell);
  const fr k = load_le(a.k + 4u * (size_t)p), r_k = load_le(bl + 16u);
  const uint32_t rs = cg1sscalar::SHARED_BASES + p * 2u * ell;
  for (uint32_t j = tid; j < ell; j += SH_THREADS) cg1sscalar::elem_terms(ell, rs, j, load_le(va + 4u * j), k, r_k, ss_tb, ss_sc);
  if (tid < 4u) cg1sscalar::blinder_terms(ell, tid, load_le(bl + 4u * tid), ss_tb, ss_sc);
}

}  // namespace cg1shuffle
