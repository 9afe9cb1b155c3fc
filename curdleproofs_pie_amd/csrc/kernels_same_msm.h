// k_smsm_step: everything of the same-MSM argument's prover (same_msm.py:73-143) that is NOT a group operation, as the kernel that sits
// between two MSM launches -- k_table_msm over the CRS table for the A side (FixedPlan) and over the proof's light table (LightPlan) for T and U, each
// with its k_fixed_finish -- so that the whole argument is one launch chain with one host wait.
// Part of the single translation unit csrc/msm_gpu.hip (after kernels_merlin.h and kernels_fixed.h).
//
// One workgroup per prover, three phases (the host enqueues  begin, table build | MSMs finish stepB | (MSMs finish round) x lg n):
//   begin    the caller's canonical scalars -> Montgomery state (x, k = 1) and the terms of B_a, B_t, B_u
//   stepB    B_a, B_t, B_u into the proof; the transcript absorbs the third same_msm_step1 list [B_a, B_t, B_u] (the first two lists
//            depend on nothing the device computes: the C entry absorbs them on the host into the states it uploads) and draws
//            same_msm_alpha; x <- r + alpha x; the terms of round 0
//   round    the six encodings into the proof; the transcript absorbs same_msm_loop [L_A, L_T, L_U, R_A, R_T, R_U] and draws
//            same_msm_gamma; gamma^-1 (fr_inv_binary); the fold; then the terms of the next round, or x_final after the last one
// The schedule and the folds are same_msm_rounds.h (shared with the host); the transcript, the status merge and the clocks are the step
// skeleton of kernels_chain.h.
#pragma once
#include "same_msm_rounds.h"
#include "kernels_chain.h"

namespace cg1smsm {

constexpr uint32_t SMSM_THREADS = 256;
constexpr uint32_t SMSM_ROW = 288;           // a prover's data row: the six (or three) encodings of a step in the transcript's order
constexpr uint32_t SMSM_BEGIN = 0, SMSM_STEPB = 1, SMSM_ROUND = 2;

struct SmsmArgs {
  uint32_t n0, lg;
  const uint32_t* gi;                        // [P][n0]
  const uint64_t* vx; const uint64_t* vr;    // [P][n0] canonical scalars
  fr* x; fr* k;                              // the state: [P][n0] each
  uint8_t* states;                           // [P][208]
  uint8_t* row;                              // [P][SMSM_ROW]
  uint8_t* chal;                             // [P][32]: where the transcript writes its draw
  const uint32_t* pts_a;                     // k_fixed_finish's encodings of the launch over G:     [P][1 or 2][12 words]
  const uint32_t* pts_tu;                    // k_fixed_finish's encodings of the launch over T | U: [P][2 or 4][12 words]
  uint32_t* proof; uint32_t proof_words;     // [P][proof_words]: SameMSMProof.to_bytes order
  uint32_t* tba; uint64_t* sca;              // the term arrays k_table_msm<FixedPlan> reads
  uint32_t* tbl; uint64_t* scl;              // the term arrays k_table_msm<LightPlan> reads
  const uint32_t* status_a; const uint32_t* status_tu;     // the status words of the two MSM launches before
  uint32_t* chain_status;                    // accumulated over the chain, read once at its end
  uint32_t* clocks;                          // [P][4]: lane 0's clock ticks (s_memtime) in the transcript | the inversions of gamma | whole steps that emit terms | steps counted
};

__global__ void __launch_bounds__(SMSM_THREADS) k_smsm_step(SmsmArgs a, uint32_t phase, uint32_t len, uint32_t round) {
  __shared__ cg1chain::StepLds s;                // (its fifth label slot is unused here)

  const uint32_t tid = threadIdx.x, p = blockIdx.x, n0 = a.n0, h = n0 / 2u;
  const unsigned long long t_in = __builtin_amdgcn_s_memtime();
  const size_t vo = (size_t)p * n0;
  View v;
  v.x = a.x + vo; v.k = a.k + vo; v.gi = a.gi + vo; v.tu = p * 2u * n0; v.n0 = n0;
  const uint64_t* vr = a.vr + 4u * vo;
  uint32_t* tba = a.tba + (size_t)p * a_terms(n0);
  uint64_t* sca = a.sca + 4u * (size_t)p * a_terms(n0);
  uint32_t* tbl = a.tbl + (size_t)p * tu_terms(n0);
  uint64_t* scl = a.scl + 4u * (size_t)p * tu_terms(n0);

  if (phase == SMSM_BEGIN) {
    for (uint32_t j = tid; j < n0; j += SMSM_THREADS) {
      v.x[j] = load_le(a.vx + 4u * (vo + j));
      v.k[j] = cg1fr::fr_one();
      begin_term(v, j, load_le(vr + 4u * j), tba, sca, tbl, scl);
    }
    return;
  }

  // ---- the encodings of the two launches before: into the proof and, in the transcript's order, into the data row
  uint32_t* proof = a.proof + (size_t)p * a.proof_words;
  const uint32_t npts = phase == SMSM_STEPB ? 3u : 6u;
  uint8_t* row = a.row + (size_t)p * SMSM_ROW;
  if (tid < npts * 12u) {
    const uint32_t q = tid / 12u, w = tid - q * 12u, g = q / 3u, m = q - 3u * g;      // g: L or R; m: A, T, U
    const uint32_t val = m == 0u ? a.pts_a[((size_t)p * (npts / 3u) + g) * 12u + w] : a.pts_tu[((size_t)p * 2u * (npts / 3u) + 2u * g + m - 1u) * 12u + w];
    // SameMSMProof.to_bytes: B_a | B_t | B_u | vec_L_A | vec_L_T | vec_L_U | vec_R_A | vec_R_T | vec_R_U | x_final
    const uint32_t slot = phase == SMSM_STEPB ? q : 3u + q * a.lg + round;
    proof[slot * 12u + w] = val;
    reinterpret_cast<uint32_t*>(row)[tid] = val;
  }
  // ---- the transcript, on lane 0
  if (tid == 64u) {
    using cg1chain::label; using cg1chain::op;
    label(s.labels, "same_msm_step1", 14); label(s.labels + 8, "same_msm_alpha", 14);
    label(s.labels + 16, "same_msm_loop", 13); label(s.labels + 24, "same_msm_gamma", 14);
    if (phase == SMSM_STEPB) {
      for (uint32_t q = 0; q < 3u; ++q) s.ops[q] = op(cg1merlin::OP_APPEND_POINT, 0, 14, 48, 48u * q, 0);
      s.ops[3] = op(cg1merlin::OP_CHALLENGE_SCALAR, 1, 14, 32, 0, 0);   // alpha
    } else {
      for (uint32_t q = 0; q < 6u; ++q) s.ops[q] = op(cg1merlin::OP_APPEND_POINT, 2, 13, 48, 48u * q, 0);
      s.ops[6] = op(cg1merlin::OP_CHALLENGE_SCALAR, 3, 14, 32, 0, 0);   // gamma
    }
  }
  const bool first = phase == SMSM_STEPB;
  uint32_t* ck = a.clocks ? a.clocks + 4u * p : nullptr;
  cg1chain::transcript_step(s, a.states + (size_t)p * 208, first ? 4u : 7u, row, a.chal + (size_t)p * 32, a.status_a, a.status_tu, a.chain_status,
                            first ? cg1chain::INV_NONE : cg1chain::INV_BINARY, nullptr, ck);

  // ---- the Fr step
  uint32_t cur = len;                                                   // the vector's length once this step is done
  if (phase == SMSM_STEPB) {
    const fr alpha = s.ch[0];
    for (uint32_t j = tid; j < n0; j += SMSM_THREADS) blind_elem(v, j, alpha, load_le(vr + 4u * j));
  } else {
    const fr gamma = s.ch[0], gamma_inv = s.ch[1];
    cur = len / 2u;
    for (uint32_t t = tid; t < h; t += SMSM_THREADS) fold_elem(v, cur, t, gamma, gamma_inv);
  }
  __threadfence_block();
  __syncthreads();
  if (cur == 1u) {                                                      // after the last fold: x_final
    if (tid == 0u) cg1chain::put_scalar(proof + (3u + 6u * a.lg) * 12u, v.x[0]);
    return;
  }
  // ---- the terms of the next round
  const uint32_t half = cur / 2u;
  for (uint32_t t = tid; t < h; t += SMSM_THREADS) round_term(v, half, t, tba, sca, tbl, scl);
  if (tid == 0u) cg1chain::step_clock(ck, t_in);
}

}  // namespace cg1smsm
