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
// and the transcript on lane 0 -- cg1merlin::Machine over the prover's OWN 208-byte state (loaded from and written back to device
// memory), reading the encodings where k_fixed_finish wrote them.  The serial part of a step is that lane: the Keccak permutations
// of five absorbs and a rejection-sampled draw, then the inversion of gamma; its shader clocks are reported per prover.
#pragma once
#include "ipa_rounds.h"

namespace cg1ipa {
using cg1merlin::COp;
using cg1merlin::LANES;
using cg1merlin::Machine;

constexpr uint32_t IPA_THREADS = 256;
constexpr uint32_t IPA_TROW = 224;           // a prover's step-1 data row: C | D | z | B_c | B_d
constexpr uint32_t IPA_BEGIN = 0, IPA_STEP1 = 1, IPA_ROUND = 2;

struct IpaArgs {
  uint32_t n0, lg, has_coeffs, inv_fermat;
  const uint32_t* gi; const uint32_t* gpi; const uint32_t* hi;         // [P][n0], [P][n0], [P]
  const uint64_t* coef; const uint64_t* vc; const uint64_t* vd; const uint64_t* rc; const uint64_t* rd;   // [P][n0] canonical scalars
  fr* c; fr* d; fr* kG; fr* kGp; fr* kH;     // the state: [P][n0] each, [P]
  uint8_t* states;                           // [P][208]
  uint8_t* trow;                             // [P][IPA_TROW]
  uint8_t* chal;                             // [P][64]: where the transcript writes its draws
  const uint32_t* pts48;                     // k_fixed_finish's encodings of the launch before: [P][2 or 4][12 words]
  uint32_t* proof; uint32_t proof_words;     // [P][proof_words]: IPA.to_bytes order
  uint32_t* tb; uint64_t* sc;                // the term arrays k_table_msm reads: indices, scalars
  const uint32_t* msm_status;                // the status word of the MSM launch before
  uint32_t* chain_status;                    // accumulated over the chain, read once at its end
  uint32_t* clocks;                          // [P][4]: lane 0's clock ticks (s_memtime) in the transcript | the inversions of gamma | whole steps that emit terms | steps counted
};

__device__ __noinline__ fr ipa_inv_fermat(const fr& a) { return cg1fr::fr_inv(a); }
__device__ __noinline__ fr ipa_inv_binary(const fr& a) { return fr_inv_binary(a); }

__device__ inline void ipa_label(uint32_t* dst, const char* s, uint32_t n) {      // label words, little-endian, zero-padded to 32 bytes
  for (uint32_t j = 0; j < 8u; ++j) dst[j] = 0u;
  for (uint32_t j = 0; j < n; ++j) dst[j >> 2] |= (uint32_t)(uint8_t)s[j] << ((j & 3u) * 8u);
}
__device__ inline COp ipa_op(uint32_t kind, uint32_t label, uint32_t llen, uint32_t len, uint32_t data_off, uint32_t out_off) {
  COp o;
  o.kind_label = kind | (label << 8) | (llen << 16);
  o.len = len; o.data_off = data_off; o.out_off = out_off;
  return o;
}

__global__ void __launch_bounds__(IPA_THREADS) k_ipa_step(IpaArgs a, uint32_t phase, uint32_t len, uint32_t round) {
  __shared__ uint32_t s_sponge[52 * LANES];
  __shared__ uint32_t s_drawn[8 * LANES];
  __shared__ uint32_t s_labels[5 * 8];
  __shared__ uint32_t s_inf[12];
  __shared__ COp s_ops[8];
  __shared__ fr s_red[2][IPA_THREADS];
  __shared__ fr s_ch[2];

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
  const uint32_t npts = phase == IPA_STEP1 ? 2u : 4u;
  const uint32_t* pts = a.pts48 + (size_t)p * npts * 12u;
  uint8_t* trow = a.trow + (size_t)p * IPA_TROW;
  if (tid < npts * 12u) {
    const uint32_t q = tid / 12u, w = tid - q * 12u, val = pts[tid];
    // IPA.to_bytes: B_c | B_d | vec_L_C | vec_R_C | vec_L_D | vec_R_D | c_final | d_final; a round's four are L_C, L_D, R_C, R_D
    const uint32_t slot = phase == IPA_STEP1 ? q : 2u + (q == 0u ? 0u : q == 1u ? 2u : q == 2u ? 1u : 3u) * a.lg + round;
    proof[slot * 12u + w] = val;
    if (phase == IPA_STEP1) reinterpret_cast<uint32_t*>(trow + 128)[tid] = val;
  }
  // ---- the transcript, on lane 0
  uint8_t* st = a.states + (size_t)p * 208;
  if (tid < 50u) s_sponge[tid * LANES] = reinterpret_cast<const uint32_t*>(st)[tid];
  if (tid == 64u) {
    ipa_label(s_labels, "ipa_step1", 9); ipa_label(s_labels + 8, "ipa_alpha", 9); ipa_label(s_labels + 16, "ipa_beta", 8);
    ipa_label(s_labels + 24, "ipa_loop", 8); ipa_label(s_labels + 32, "ipa_gamma", 9);
    s_inf[0] = 0xC0u;                                                   // the canonical encoding of the identity: C0 00 .. 00
    for (int j = 1; j < 12; ++j) s_inf[j] = 0u;
    if (phase == IPA_STEP1) {
      s_ops[0] = ipa_op(cg1merlin::OP_APPEND_POINT, 0, 9, 48, 0, 0);    // C
      s_ops[1] = ipa_op(cg1merlin::OP_APPEND_POINT, 0, 9, 48, 48, 0);   // D
      s_ops[2] = ipa_op(cg1merlin::OP_APPEND, 0, 9, 32, 96, 0);         // z
      s_ops[3] = ipa_op(cg1merlin::OP_APPEND_POINT, 0, 9, 48, 128, 0);  // B_c
      s_ops[4] = ipa_op(cg1merlin::OP_APPEND_POINT, 0, 9, 48, 176, 0);  // B_d
      s_ops[5] = ipa_op(cg1merlin::OP_CHALLENGE_SCALAR, 1, 9, 32, 0, 0);
      s_ops[6] = ipa_op(cg1merlin::OP_CHALLENGE_SCALAR, 2, 8, 32, 0, 32);
    } else {
      for (uint32_t q = 0; q < 4u; ++q) s_ops[q] = ipa_op(cg1merlin::OP_APPEND_POINT, 3, 8, 48, 48u * q, 0);
      s_ops[4] = ipa_op(cg1merlin::OP_CHALLENGE_SCALAR, 4, 9, 32, 0, 0);
    }
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0u) {
    if (a.msm_status[0] != 0u) atomicOr(a.chain_status, a.msm_status[0]);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    Machine m;
    m.w = s_sponge; m.drawn = s_drawn; m.labels = s_labels; m.consts = reinterpret_cast<const uint8_t*>(s_inf);
    m.pos = st[200]; m.pos_begin = st[201]; m.cur_flags = st[202];
    m.k = 0; m.ph = 0; m.i = 0; m.hdr = 0; m.stage = 0; m.k_loaded = 0xffffffffu; m.rec = make_uint4(0, 0, 0, 0);
    const uint8_t* row = phase == IPA_STEP1 ? trow : reinterpret_cast<const uint8_t*>(pts);
    uint8_t* orow = a.chal + (size_t)p * 64;
    const uint32_t nops = phase == IPA_STEP1 ? 7u : 5u;
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
    if (phase == IPA_STEP1) a.kH[p] = load_le(reinterpret_cast<const uint64_t*>(orow + 32));      // beta
    else s_ch[1] = a.inv_fermat ? ipa_inv_fermat(ch) : ipa_inv_binary(ch);
    const unsigned long long t2 = __builtin_amdgcn_s_memtime();
    if (a.clocks) {
      uint32_t* ck = a.clocks + 4u * p;
      ck[0] += (uint32_t)(t1 - t0);
      if (phase == IPA_ROUND) ck[1] += (uint32_t)(t2 - t1);
      ck[3] += 1u;
    }
  }
  __threadfence_block();
  __syncthreads();
  if (tid < 50u) reinterpret_cast<uint32_t*>(st)[tid] = s_sponge[tid * LANES];

  // ---- the Fr step
  uint32_t cur = len;                                                   // the vectors' length once this step is done
  if (phase == IPA_STEP1) {
    const fr alpha = s_ch[0];
    for (uint32_t j = tid; j < n0; j += IPA_THREADS) blind_elem(v, j, alpha, load_le(rc + 4u * j), load_le(rd + 4u * j));
  } else {
    const fr gamma = s_ch[0], gamma_inv = s_ch[1];
    cur = len / 2u;
    for (uint32_t t = tid; t < h; t += IPA_THREADS) fold_elem(v, cur, t, gamma, gamma_inv);
  }
  __threadfence_block();
  __syncthreads();
  if (cur == 1u) {                                                      // after the last fold: c_final | d_final
    if (tid < 2u) {
      uint64_t w[4];
      cg1fr::fr_to_le32(tid == 0u ? v.c[0] : v.d[0], reinterpret_cast<uint8_t*>(w));
      uint32_t* dst = proof + (2u + 4u * a.lg) * 12u + 8u * tid;
      for (int k = 0; k < 4; ++k) { dst[2 * k] = (uint32_t)w[k]; dst[2 * k + 1] = (uint32_t)(w[k] >> 32); }
    }
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
    if (a.clocks) a.clocks[4u * p + 2u] += (uint32_t)(__builtin_amdgcn_s_memtime() - t_in);
  }
}

}  // namespace cg1ipa
