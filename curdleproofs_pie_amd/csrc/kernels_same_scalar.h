// k_sscalar_step: everything of the shuffle prover's same-scalar block (curdleproofs.py:92-116, same_scalar.py:39-69) that is NOT a group
// operation, as the kernel on both sides of the block's ONE MSM launch -- k_table_msm<LightPlan> over the call's light table of
// G_t | G_u | H | the provers' vec_R | vec_S, ten MSMs per prover, and its k_fixed_finish -- so that R, S, cm_T, cm_U and the whole of
// SameScalarProof.new are one launch chain with one host wait.
// Part of the single translation unit csrc/msm_gpu.hip (after kernels_merlin.h and kernels_fixed.h).
//
// One workgroup per prover, two phases (the host enqueues  begin | table build | [k_subgroup_row] | MSMs finish | step):
//   begin    the caller's canonical scalars -> Montgomery form, k a_i and r_k a_i on all lanes (lane t owns elements t, t + 256, ...), the
//            base indices and canonical scalars of the ten MSMs in the transcript's order
//   step     the ten encodings into the proof; the transcript absorbs sameexp_points [R, S, T.T_1, T.T_2, U.T_1, U.T_2, A.T_1, A.T_2,
//            B.T_1, B.T_2] and draws same_scalar_alpha; z_k, z_t, z_u.  k_fixed_finish left the encodings in exactly that order: they
//            ARE the transcript's data row.  The flags k_subgroup_row left for vec_R | vec_S (when the caller did not certify them) are
//            reduced here into the chain's status word: the folded scalars are exact only for bases of order r
// The schedule and the formulas are same_scalar_rounds.h (shared with the host); the transcript, the status merge and the clocks are the
// step skeleton of kernels_chain.h.
#pragma once
#include "same_scalar_rounds.h"
#include "kernels_chain.h"

namespace cg1sscalar {

constexpr uint32_t SS_THREADS = 256;
constexpr uint32_t SS_BEGIN = 0, SS_STEP = 1;
constexpr uint32_t SS_ROW = MSMS * 48u;      // a prover's data row: k_fixed_finish's ten encodings

struct SscalarArgs {
  uint32_t ell;
  const uint64_t* va;                        // [P][ell] canonical scalars: vec_a
  const uint64_t* k;                         // [P] canonical
  const uint64_t* bl;                        // [P][5] canonical: r_t r_u r_a r_b r_k
  uint8_t* states;                           // [P][208]
  uint8_t* chal;                             // [P][32]: where the transcript writes its draw
  const uint32_t* pts;                       // k_fixed_finish's encodings: [P][MSMS][12 words]
  uint32_t* proof;                           // [P][PROOF_BYTES / 4]: cm_T | cm_U | R | S | cm_A | cm_B | z_k | z_t | z_u
  uint32_t* tb; uint64_t* sc;                // the term arrays k_table_msm<LightPlan> reads: [P][terms(ell)]
  const uint8_t* in_g1;                      // nullable: k_subgroup_row's flags of vec_R | vec_S, [P][2 ell]
  const uint32_t* status_msm;                // the status word of the MSM launch before
  uint32_t* chain_status;                    // accumulated over the chain, read once at its end
  uint32_t* clocks;                          // [P][4]: lane 0's clock ticks (s_memtime) in the transcript | unused | unused | transcript programs counted
};

__global__ void __launch_bounds__(SS_THREADS) k_sscalar_step(SscalarArgs a, uint32_t phase) {
  __shared__ cg1chain::StepLds s;

  const uint32_t tid = threadIdx.x, p = blockIdx.x, ell = a.ell;
  const uint64_t* bl = a.bl + 20u * (size_t)p;

  if (phase == SS_BEGIN) {
    const uint64_t* va = a.va + 4u * (size_t)p * ell;
    uint32_t* tb = a.tb + (size_t)p * terms(ell);
    uint64_t* sc = a.sc + 4u * (size_t)p * terms(ell);
    const fr k = load_le(a.k + 4u * (size_t)p), r_k = load_le(bl + 16u);
    const uint32_t rs = SHARED_BASES + p * 2u * ell;
    for (uint32_t j = tid; j < ell; j += SS_THREADS) elem_terms(ell, rs, j, load_le(va + 4u * j), k, r_k, tb, sc);
    if (tid < 4u) blinder_terms(ell, tid, load_le(bl + 4u * tid), tb, sc);
    return;
  }

  // ---- a base outside G1: the chain runs on, the call is refused at its end
  if (a.in_g1) {
    const uint8_t* fl = a.in_g1 + (size_t)p * 2u * ell;
    uint32_t bad = 0;
    for (uint32_t j = tid; j < 2u * ell; j += SS_THREADS) bad |= fl[j] ? 0u : ST_NOT_G1;
    if (bad) atomicOr(a.chain_status, bad);
  }
  // ---- the encodings of the launch before: into the proof
  const uint32_t* pts = a.pts + (size_t)p * (SS_ROW / 4u);
  uint32_t* proof = a.proof + (size_t)p * (PROOF_BYTES / 4u);
  if (tid < SS_ROW / 4u) {
    const uint32_t q = tid / 12u, w = tid - q * 12u;
    proof[proof_slot(q) * 12u + w] = pts[tid];
  }
  // ---- the transcript, on lane 0.  StepLds holds eight op records: the list of ten goes as two programs, eight appends, then two and
  // the draw -- one append_list all the same (a list is its items under one label, curdleproofs_transcript.py)
  const uint8_t* row = reinterpret_cast<const uint8_t*>(pts);
  uint8_t* st = a.states + (size_t)p * 208;
  uint8_t* chal = a.chal + (size_t)p * 32;
  uint32_t* ck = a.clocks ? a.clocks + 4u * p : nullptr;
  using cg1chain::label; using cg1chain::op;
#pragma unroll 1
  for (uint32_t first = 0; first < MSMS; first += 8u) {
    const uint32_t appends = MSMS - first < 8u ? MSMS - first : 8u;
    const bool draw = first + appends == MSMS;
    if (tid == 64u) {
      label(s.labels, "sameexp_points", 14); label(s.labels + 8, "same_scalar_alpha", 17);
      for (uint32_t q = 0; q < appends; ++q) s.ops[q] = op(cg1merlin::OP_APPEND_POINT, 0, 14, 48, 48u * (first + q), 0);
      if (draw) s.ops[appends] = op(cg1merlin::OP_CHALLENGE_SCALAR, 1, 17, 32, 0, 0);       // alpha
    }
    cg1chain::transcript_step(s, st, appends + (draw ? 1u : 0u), row, chal, a.status_msm, nullptr, a.chain_status, cg1chain::INV_NONE, nullptr, ck);
    __syncthreads();                                                    // (lane 64 rewrites the op records the next program reads)
  }

  // ---- the responses (same_scalar.py:65-67): lane 0 z_k = r_k + k alpha, lane 1 z_t = r_a + r_t alpha, lane 2 z_u = r_b + r_u alpha
  if (tid < 3u) {
    const fr alpha = s.ch[0];
    const uint64_t* blinder = bl + (tid == 0u ? 16u : 4u + 4u * tid);
    const uint64_t* secret = tid == 0u ? a.k + 4u * (size_t)p : bl + 4u * (tid - 1u);
    cg1chain::put_scalar(proof + MSMS * 12u + 8u * tid, response(load_le(blinder), load_le(secret), alpha));
  }
}

}  // namespace cg1sscalar
