// k_smsm_step: everything of the same-MSM argument's prover (same_msm.py:73-143) that is NOT a group operation, as the kernel that sits
// between two MSM launches -- k_table_msm over the CRS table for the A side (FixedPlan) and over the proof's light table (LightPlan) for T and U, each
// with its k_fixed_finish -- so that the whole argument is one launch chain with one host wait.
// Part of the single translation unit csrc/msm_gpu.hip (after kernels_ipa.h, whose label / op helpers it reuses).
//
// One workgroup per prover, three phases (the host enqueues  begin, table build | MSMs finish stepB | (MSMs finish round) x lg n):
//   begin    the caller's canonical scalars -> Montgomery state (x, k = 1) and the terms of B_a, B_t, B_u
//   stepB    B_a, B_t, B_u into the proof; the transcript absorbs the third same_msm_step1 list [B_a, B_t, B_u] (the first two lists
//            depend on nothing the device computes: the C entry absorbs them on the host into the states it uploads) and draws
//            same_msm_alpha; x <- r + alpha x; the terms of round 0
//   round    the six encodings into the proof; the transcript absorbs same_msm_loop [L_A, L_T, L_U, R_A, R_T, R_U] and draws
//            same_msm_gamma; gamma^-1 (fr_inv_binary); the fold; then the terms of the next round, or x_final after the last one
// The schedule and the folds are same_msm_rounds.h (shared with the host); the transcript runs on lane 0 as in k_ipa_step.
#pragma once
#include "same_msm_rounds.h"

namespace cg1smsm {
using cg1merlin::COp;
using cg1merlin::LANES;
using cg1merlin::Machine;

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
  __shared__ uint32_t s_sponge[52 * LANES];
  __shared__ uint32_t s_drawn[8 * LANES];
  __shared__ uint32_t s_labels[4 * 8];
  __shared__ uint32_t s_inf[12];
  __shared__ COp s_ops[8];
  __shared__ fr s_ch[2];

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
  uint8_t* st = a.states + (size_t)p * 208;
  if (tid < 50u) s_sponge[tid * LANES] = reinterpret_cast<const uint32_t*>(st)[tid];
  if (tid == 64u) {
    cg1ipa::ipa_label(s_labels, "same_msm_step1", 14); cg1ipa::ipa_label(s_labels + 8, "same_msm_alpha", 14);
    cg1ipa::ipa_label(s_labels + 16, "same_msm_loop", 13); cg1ipa::ipa_label(s_labels + 24, "same_msm_gamma", 14);
    s_inf[0] = 0xC0u;                                                   // the canonical encoding of the identity: C0 00 .. 00
    for (int j = 1; j < 12; ++j) s_inf[j] = 0u;
    if (phase == SMSM_STEPB) {
      for (uint32_t q = 0; q < 3u; ++q) s_ops[q] = cg1ipa::ipa_op(cg1merlin::OP_APPEND_POINT, 0, 14, 48, 48u * q, 0);
      s_ops[3] = cg1ipa::ipa_op(cg1merlin::OP_CHALLENGE_SCALAR, 1, 14, 32, 0, 0);
    } else {
      for (uint32_t q = 0; q < 6u; ++q) s_ops[q] = cg1ipa::ipa_op(cg1merlin::OP_APPEND_POINT, 2, 13, 48, 48u * q, 0);
      s_ops[6] = cg1ipa::ipa_op(cg1merlin::OP_CHALLENGE_SCALAR, 3, 14, 32, 0, 0);
    }
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0u) {
    const uint32_t bad = a.status_a[0] | a.status_tu[0];
    if (bad != 0u) atomicOr(a.chain_status, bad);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    Machine m;
    m.w = s_sponge; m.drawn = s_drawn; m.labels = s_labels; m.consts = reinterpret_cast<const uint8_t*>(s_inf);
    m.pos = st[200]; m.pos_begin = st[201]; m.cur_flags = st[202];
    m.k = 0; m.ph = 0; m.i = 0; m.hdr = 0; m.stage = 0; m.k_loaded = 0xffffffffu; m.rec = make_uint4(0, 0, 0, 0);
    uint8_t* orow = a.chal + (size_t)p * 32;
    const uint32_t nops = phase == SMSM_STEPB ? 4u : 7u;
    bool done = false;
    for (;;) {
      bool blocked = false;
      if (!m.advance(s_ops, nops, row, orow, done, blocked)) break;
      cg1merlin::keccak_words(m.w);
      m.pos = 0; m.pos_begin = 0;
    }
    st[200] = (uint8_t)m.pos; st[201] = (uint8_t)m.pos_begin; st[202] = (uint8_t)m.cur_flags;
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    const fr ch = load_le(reinterpret_cast<const uint64_t*>(orow));     // alpha, or gamma
    s_ch[0] = ch;
    if (phase == SMSM_ROUND) s_ch[1] = cg1ipa::ipa_inv_binary(ch);
    const unsigned long long t2 = __builtin_amdgcn_s_memtime();
    if (a.clocks) {
      uint32_t* ck = a.clocks + 4u * p;
      ck[0] += (uint32_t)(t1 - t0);
      if (phase == SMSM_ROUND) ck[1] += (uint32_t)(t2 - t1);
      ck[3] += 1u;
    }
  }
  __threadfence_block();
  __syncthreads();
  if (tid < 50u) reinterpret_cast<uint32_t*>(st)[tid] = s_sponge[tid * LANES];

  // ---- the Fr step
  uint32_t cur = len;                                                   // the vector's length once this step is done
  if (phase == SMSM_STEPB) {
    const fr alpha = s_ch[0];
    for (uint32_t j = tid; j < n0; j += SMSM_THREADS) blind_elem(v, j, alpha, load_le(vr + 4u * j));
  } else {
    const fr gamma = s_ch[0], gamma_inv = s_ch[1];
    cur = len / 2u;
    for (uint32_t t = tid; t < h; t += SMSM_THREADS) fold_elem(v, cur, t, gamma, gamma_inv);
  }
  __threadfence_block();
  __syncthreads();
  if (cur == 1u) {                                                      // after the last fold: x_final
    if (tid == 0u) {
      uint64_t w[4];
      cg1fr::fr_to_le32(v.x[0], reinterpret_cast<uint8_t*>(w));
      uint32_t* dst = proof + (3u + 6u * a.lg) * 12u;
      for (int k = 0; k < 4; ++k) { dst[2 * k] = (uint32_t)w[k]; dst[2 * k + 1] = (uint32_t)(w[k] >> 32); }
    }
    return;
  }
  // ---- the terms of the next round
  const uint32_t half = cur / 2u;
  for (uint32_t t = tid; t < h; t += SMSM_THREADS) round_term(v, half, t, tba, sca, tbl, scl);
  if (tid == 0u && a.clocks) a.clocks[4u * p + 2u] += (uint32_t)(__builtin_amdgcn_s_memtime() - t_in);
}

}  // namespace cg1smsm
