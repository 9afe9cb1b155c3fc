// k_same_perm_begin: the head of the same-permutation argument's prover (same_perm.py:48-59) in front of the grand-product launch chain --
// so that SamePermutationProof.new is that chain with another first kernel, still one host wait:
//     k_same_perm_begin | MSM finish | k_gprod_step step (same_perm) | MSM finish | k_ipa_step step1 | (MSM finish k_ipa_step round) x lg n
// Part of the single translation unit csrc/msm_gpu.hip (after kernels_gprod.h).
//
// One workgroup per prover, as k_gprod_step's begin phase, which it replaces: with same_perm_alpha and same_perm_beta drawn on the host
// (they depend on nothing the device computes) it gathers vec_a[perm[i]], forms b | b_blinders into the buffer the step phase reads as
// vb, scans the prefix products c, WRITES gprod_result = c[ell-1] b[ell-1] into the data row (computed here, not checked) and emits the
// terms of A' | M' | B' | C (same_perm_rounds.h, shared with the host).  The step phase compares A' and M' with the caller's A and M and
// emits B' as B.  The host has refused perm[i] >= ell before the launch.  Its own kernel rather than a third phase of k_gprod_step: that
// kernel's registers and scratch stay what they were.
#pragma once
#include "kernels_gprod.h"

namespace cg1sperm {
using cg1gprod::GP_THREADS;

struct SamePermArgs {
  cg1gprod::GprodArgs g;                     // the chain's arguments (same_perm = 1): c, gi, cbl, row, the term arrays
  const uint64_t* va;                        // [P][ell] canonical: vec_a
  const uint32_t* perm;                      // [P][ell], every entry < ell
  const uint64_t* abl; const uint64_t* mbl;  // [P][nb] canonical each: vec_a_blinders, vec_m_blinders
  const uint64_t* ab;                        // [P][2] canonical: same_perm_alpha | same_perm_beta
  uint64_t* vb;                              // [P][n0] canonical, written here: b | b_blinders (= g.vb)
};

__global__ void __launch_bounds__(GP_THREADS) k_same_perm_begin(SamePermArgs a) {
  __shared__ fr s_scan[GP_THREADS];

  const uint32_t tid = threadIdx.x, p = blockIdx.x, n = a.g.ipa.n0, ell = a.g.ell, nb = a.g.nb;
  const size_t vo = (size_t)p * n;
  fr* c = a.g.ipa.c + vo;
  const uint32_t* gi = a.g.ipa.gi + vo;
  const uint64_t* va = a.va + 4u * (size_t)p * ell;
  const uint32_t* perm = a.perm + (size_t)p * ell;
  const uint64_t* abl = a.abl + 4u * (size_t)p * nb;
  const uint64_t* mbl = a.mbl + 4u * (size_t)p * nb;
  const uint64_t* cbl = a.g.cbl + 4u * (size_t)p * nb;
  uint64_t* vb = a.vb + 4u * vo;
  uint8_t* row = a.g.row + (size_t)p * cg1gprod::GP_ROW;
  const fr alpha = load_le(a.ab + 8u * (size_t)p), beta = load_le(a.ab + 8u * (size_t)p + 4u);

  // ---- b | b_blinders, canonical, where the step phase reads them
  for (uint32_t j = tid; j < n; j += GP_THREADS) {
    fr b;
    if (j < ell) {
      const uint32_t m = perm[j];
      b = factor(load_le(va + 4u * m), m, alpha, beta);
    } else {
      b = blinder(load_le(abl + 4u * (j - ell)), load_le(mbl + 4u * (j - ell)), alpha);
    }
    cg1fr::fr_to_le32(b, reinterpret_cast<uint8_t*>(vb + 4u * j));
  }
  __threadfence_block();
  __syncthreads();
  // ---- the prefix products c and gprod_result
  cg1gprod::scan_products(s_scan, ell, [&](uint32_t i) { return load_le(vb + 4u * i); },
                          [&](uint32_t i, const fr& pre) {
                            c[i] = pre;
                            if (i == ell - 1u) cg1fr::fr_to_le32(cg1fr::fr_mul(pre, load_le(vb + 4u * i)), row + 48);
                          });
  for (uint32_t k = tid; k < nb; k += GP_THREADS) c[ell + k] = load_le(cbl + 4u * k);
  __threadfence_block();
  __syncthreads();
  // ---- the terms of A', M', B', C
  uint32_t* tb = a.g.ipa.tb + (size_t)p * begin_terms(n);
  uint64_t* sc = a.g.ipa.sc + 4u * (size_t)p * begin_terms(n);
  for (uint32_t j = tid; j < n; j += GP_THREADS) {
    fr aj, mj;
    if (j < ell) {
      const uint32_t m = perm[j];
      aj = load_le(va + 4u * m); mj = cg1fr::fr_from_u64(m);
    } else {
      aj = load_le(abl + 4u * (j - ell)); mj = load_le(mbl + 4u * (j - ell));
    }
    begin_term(gi, n, j, aj, mj, load_le(vb + 4u * j), c[j], tb, sc);
  }
}

}  // namespace cg1sperm
