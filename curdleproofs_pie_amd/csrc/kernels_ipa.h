// k_ipa_step: everything of the inner-product argument's prover (ipa.py:97-153) that is NOT a group operation, as the kernel that
// sits between two k_table_msm / k_fixed_finish launches -- so that the whole argument is one launch chain with one host wait.
// Part of the single translation unit csrc/msm_gpu.hip (after kernels_merlin.h and kernels_fixed.h).
//
// One workgroup per prover, three phases (the host enqueues  begin | MSM finish step1 | (MSM finish round) x lg n):
//   begin    the caller's canonical scalars -> Montgomery state (c, d, kG = 1, kGp = the G' coefficients or 1) and the terms of
//            B_c = MSM(G, r_c), B_d = MSM(G', r_d)
//   step1    B_c, B_d into the proof; the transcript absorbs ipa_step1 [C, D], z, [B_c, B_d] and draws ipa_alpha, ipa_beta;
//            c <- r_c + alpha c, d <- r_d + alpha d; kH = beta; the terms of round 0
//   round    the four encodings k_fixed_finish left into the proof; the transcript absorbs ipa_loop [L_C, L_D, R_C, R_D] and draws
//            ipa_gamma; gamma^-1; the fold; then the terms of the next round, or c_final | d_final after the last one
// The schedule and the folds are ipa_rounds.h (shared with the host); here: one lane per term, the two inner products by an LDS tree,
// and the step skeleton of kernels_chain.h: the transcript on lane 0 (five absorbs and a rejection-sampled draw, then the inversion
// of gamma), the status merge, the clocks.
#pragma once
#include "ipa_rounds.h"
#include "kernels_chain.h"

namespace cg1ipa {

constexpr uint32_t IPA_THREADS = 256;
constexpr uint32_t IPA_TROW = 224;           // a prover's step-1 data row: C | D | z | B_c | B_d
constexpr uint32_t IPA_BEGIN = 0, IPA_STEP1 = 1, IPA_ROUND = 2;

struct IpaArgs {
  uint32_t n0, lg, has_coeffs, inv_fermat;
  uint32_t d_first = 0;                      // 1: the launch before step 1 left THREE encodings, D | B_c | B_d, and D goes into the data row (kernels_gprod.h)
  const uint32_t* gi; const uint32_t* gpi; const uint32_t* hi;         // [P][n0], [P][n0], [P]
  const uint64_t* coef; const uint64_t* vc; const uint64_t* vd; const uint64_t* rc; const uint64_t* rd;   // [P][n0] canonical scalars
  fr* c; fr* d; fr* kG; fr* kGp; fr* kH;     // the state: [P][n0] each, [P]
  uint8_t* states;                           // [P][208]
  uint8_t* trow;                             // [P][IPA_TROW]
  uint8_t* chal;                             // [P][64]: where the transcript writes its draws
  const uint32_t* pts48;                     // k_fixed_finish's encodings of the launch before: [P][2 (3 with d_first) or 4][12 words]
  uint32_t* proof; uint32_t proof_words;     // [P][proof_words]: IPA.to_bytes order
  uint32_t* tb; uint64_t* sc;                // the term arrays k_table_msm reads: indices, scalars
  const uint32_t* msm_status;                // the status word of the MSM launch before
  uint32_t* chain_status;                    // accumulated over the chain, read once at its end
  uint32_t* clocks;                          // [P][4]: lane 0's clock ticks (s_memtime) in the transcript | the inversions of gamma | whole steps that emit terms | steps counted
};

__global__ void __launch_bounds__(IPA_THREADS) k_ipa_step(IpaArgs a, uint32_t phase, uint32_t len, uint32_t round) {
  __shared__ cg1chain::StepLds s;
  __shared__ fr s_red[2][IPA_THREADS];

  const uint32_t tid = threadIdx.x, p = blockIdx.x, n0 = a.n0, h = n0 / 2u;
  const unsigned long long t_in = __builtin_amdgcn_s_memtime();
  const size_t vo = (size_t)p * n0;
  View v;
  v.c = a.c + vo; v.d = a.d + vo; v.kG = a.kG + vo; v.kGp = a.kGp + vo;
  v.gi = a.gi + vo; v.gpi = a.gpi + vo; v.hi = a.hi[p]; v.n0 = n0;
  const uint64_t* rc = a.rc + 4u * vo;
  const uint64_t* rd = a.rd + 4u * vo;

  if (phase == IPA_BEGIN) {
    uint32_t* tb = a.tb + (size_t)p * step1_terms(n0);
    uint64_t* sc = a.sc + 4u * (size_t)p * step1_terms(n0);
    for (uint32_t j = tid; j < n0; j += IPA_THREADS) {
      v.c[j] = load_le(a.vc + 4u * (vo + j));
      v.d[j] = load_le(a.vd + 4u * (vo + j));
      v.kG[j] = cg1fr::fr_one();
      v.kGp[j] = a.has_coeffs ? load_le(a.coef + 4u * (vo + j)) : cg1fr::fr_one();
      step1_term(v, j, load_le(rc + 4u * j), load_le(rd + 4u * j), tb, sc);
    }
    return;
  }

  // ---- the encodings of the launch before: into the proof (and, step 1, into the transcript's data row)
  uint32_t* proof = a.proof + (size_t)p * a.proof_words;
  const uint32_t pre = phase == IPA_STEP1 ? a.d_first : 0u;
  const uint32_t npts = phase == IPA_STEP1 ? 2u + pre : 4u;
  const uint32_t* pts = a.pts48 + (size_t)p * npts * 12u;
  uint8_t* trow = a.trow + (size_t)p * IPA_TROW;
  if (tid < npts * 12u) {
    const uint32_t q = tid / 12u, w = tid - q * 12u, val = pts[tid];
    if (q < pre) reinterpret_cast<uint32_t*>(trow + 48)[w] = val;      // D
    else {
      // IPA.to_bytes: B_c | B_d | vec_L_C | vec_R_C | vec_L_D | vec_R_D | c_final | d_final; a round's four are L_C, L_D, R_C, R_D
      const uint32_t slot = phase == IPA_STEP1 ? q - pre : 2u + (q == 0u ? 0u : q == 1u ? 2u : q == 2u ? 1u : 3u) * a.lg + round;
      proof[slot * 12u + w] = val;
      if (phase == IPA_STEP1) reinterpret_cast<uint32_t*>(trow + 128)[tid - pre * 12u] = val;
    }
  }
  // ---- the transcript, on lane 0
  if (tid == 64u) {
    using cg1chain::label; using cg1chain::op;
    label(s.labels, "ipa_step1", 9); label(s.labels + 8, "ipa_alpha", 9); label(s.labels + 16, "ipa_beta", 8);
    label(s.labels + 24, "ipa_loop", 8); label(s.labels + 32, "ipa_gamma", 9);
    if (phase == IPA_STEP1) {
      s.ops[0] = op(cg1merlin::OP_APPEND_POINT, 0, 9, 48, 0, 0);        // C
      s.ops[1] = op(cg1merlin::OP_APPEND_POINT, 0, 9, 48, 48, 0);       // D
      s.ops[2] = op(cg1merlin::OP_APPEND, 0, 9, 32, 96, 0);             // z
      s.ops[3] = op(cg1merlin::OP_APPEND_POINT, 0, 9, 48, 128, 0);      // B_c
      s.ops[4] = op(cg1merlin::OP_APPEND_POINT, 0, 9, 48, 176, 0);      // B_d
      s.ops[5] = op(cg1merlin::OP_CHALLENGE_SCALAR, 1, 9, 32, 0, 0);    // alpha
      s.ops[6] = op(cg1merlin::OP_CHALLENGE_SCALAR, 2, 8, 32, 0, 32);   // beta
    } else {
      for (uint32_t q = 0; q < 4u; ++q) s.ops[q] = op(cg1merlin::OP_APPEND_POINT, 3, 8, 48, 48u * q, 0);
      s.ops[4] = op(cg1merlin::OP_CHALLENGE_SCALAR, 4, 9, 32, 0, 0);    // gamma
    }
  }
  const bool first = phase == IPA_STEP1;
  uint32_t* ck = a.clocks ? a.clocks + 4u * p : nullptr;
  cg1chain::transcript_step(s, a.states + (size_t)p * 208, first ? 7u : 5u, first ? trow : reinterpret_cast<const uint8_t*>(pts), a.chal + (size_t)p * 64,
                            a.msm_status, nullptr, a.chain_status, first ? cg1chain::INV_NONE : a.inv_fermat ? cg1chain::INV_FERMAT : cg1chain::INV_BINARY,
                            first ? a.kH + p : nullptr, ck);

  // ---- the Fr step
  uint32_t cur = len;                                                   // the vectors' length once this step is done
  if (phase == IPA_STEP1) {
    const fr alpha = s.ch[0];
    for (uint32_t j = tid; j < n0; j += IPA_THREADS) blind_elem(v, j, alpha, load_le(rc + 4u * j), load_le(rd + 4u * j));
  } else {
    const fr gamma = s.ch[0], gamma_inv = s.ch[1];
    cur = len / 2u;
    for (uint32_t t = tid; t < h; t += IPA_THREADS) fold_elem(v, cur, t, gamma, gamma_inv);
  }
  __threadfence_block();
  __syncthreads();
  if (cur == 1u) {                                                      // after the last fold: c_final | d_final
    if (tid < 2u) cg1chain::put_scalar(proof + (2u + 4u * a.lg) * 12u + 8u * tid, tid == 0u ? v.c[0] : v.d[0]);
    return;
  }
  // ---- the terms of the next round, and its two inner products
  uint32_t* tb = a.tb + (size_t)p * round_terms(n0);
  uint64_t* sc = a.sc + 4u * (size_t)p * round_terms(n0);
  const uint32_t half = cur / 2u;
  fr sl = cg1fr::fr_zero(), sr = cg1fr::fr_zero();
  for (uint32_t t = tid; t < h; t += IPA_THREADS) {
    fr pl, pr;
    round_term(v, half, t, tb, sc, pl, pr);
    sl = cg1fr::fr_add(sl, pl); sr = cg1fr::fr_add(sr, pr);
  }
  s_red[0][tid] = sl; s_red[1][tid] = sr;
  __syncthreads();
  for (uint32_t dd = IPA_THREADS / 2u; dd >= 1u; dd >>= 1) {
    if (tid < dd) {
      s_red[0][tid] = cg1fr::fr_add(s_red[0][tid], s_red[0][tid + dd]);
      s_red[1][tid] = cg1fr::fr_add(s_red[1][tid], s_red[1][tid + dd]);
    }
    __syncthreads();
  }
  if (tid == 0u) {
    round_h_terms(v, a.kH[p], s_red[0][0], s_red[1][0], tb, sc);
    cg1chain::step_clock(ck, t_in);
  }
}

}  // namespace cg1ipa
