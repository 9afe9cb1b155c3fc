// k_gprod_step: everything of the grand-product argument's prover (grand_prod.py:29-105) that is NOT a group operation, up to the point
// where the inner-product argument takes over -- so that GrandProductProof.new is one launch chain with one host wait:
//     k_gprod_step begin | MSM finish | k_gprod_step step | MSM finish | k_ipa_step step1 | (MSM finish k_ipa_step round) x lg n
// Part of the single translation unit csrc/msm_gpu.hip (after kernels_ipa.h).
//
// One workgroup per prover, two phases:
//   begin   the prefix products c of vec_b (one workgroup scan), the check gprod_result = c[ell-1] b[ell-1], and the terms of
//           B' = MSM(vec_G, b | b_blinders) and C = MSM(vec_G, c | c_blinders)
//   step    B' against the caller's B (48 bytes; the reference's assertions hold exactly when they agree), C into the proof; the
//           transcript absorbs gprod_step1 [B, gprod_result] and draws gprod_alpha; r_p; it absorbs gprod_step2 [C, r_p] and draws
//           gprod_beta; beta^-1; the powers of beta and of beta^-1 (the same scan, twice), vec_d, the G' coefficients, inner_prod;
//           omega and delta by an LDS tree and the last two blinders (one inversion); the terms of D, B_c, B_d
// and it leaves k_ipa_step's state -- c, d, kG = 1, kGp, the data row C | . | z, r and the completed z where its step 1 reads the
// blinders -- so the IPA's step 1 and rounds run unchanged (IpaArgs::d_first: the launch before them also computed D).
// The same-permutation argument (kernels_same_perm.h) runs this chain with another first kernel: GprodArgs::same_perm selects the step
// phase's other head (four encodings; A', M' checked, B' emitted as B) and moves the proof 12 words on; the default is this header's own.
// The formulas and the term schedule are gprod_rounds.h (shared with the host).  A zero where an inverse is wanted (beta, c[n-2], the
// second denominator of generate_ipa_blinders) is tested BEFORE the inversion and sets a status bit; the chain then runs to its end on
// zeros and the host refuses the call.
#pragma once
#include "same_perm_rounds.h"
#include "kernels_ipa.h"

namespace cg1gprod {

constexpr uint32_t GP_THREADS = 256;
constexpr uint32_t GP_ROW = 160;             // a prover's data row: B | gprod_result | C | r_p
constexpr uint32_t GP_BEGIN = 0, GP_STEP = 1;

struct GprodArgs {
  cg1ipa::IpaArgs ipa;                       // the state, data row, blinders (rc = r, rd = z), term arrays, status and clocks the IPA's phases go on with
  uint32_t ell, nb;                          // n0 = ell + nb
  const uint64_t* vb;                        // [P][n0] canonical: vec_b | vec_b_blinders
  const uint64_t* cbl;                       // [P][nb] canonical: vec_c_blinders
  uint64_t* z;                               // [P][n0] canonical: the n0 - 2 drawn entries of z; the step phase completes them (= ipa.rd)
  uint8_t* row;                              // [P][GP_ROW]
  uint32_t* proof; uint32_t proof_words;     // [P][proof_words]: GrandProductProof.to_bytes order, C | r_p | the IPA's proof (= ipa.proof)
  // The same-permutation argument's head (kernels_same_perm.h: its begin kernel ran instead of the begin phase and left vb, gprod_result
  // and FOUR encodings A' | M' | B' | C).  The defaults are the grand-product argument's own launch.
  uint32_t same_perm = 0u;                   // 1: A', M' against am48, B' EMITTED as B (row, proof words 0..11), the proof 12 words further on
  const uint32_t* am48 = nullptr;            // [P][2][12] canonical encodings: the caller's A | M
};

// The exclusive prefix products of `count` elements by the whole workgroup: out(i, in(0) .. in(i-1)).  A lane owns a block of
// ceil(count / GP_THREADS) consecutive elements: their product serially, an LDS scan over the block products (only as wide as there are
// blocks), then the block again from its prefix.  lds: GP_THREADS elements, free again on return.
template <class In, class Out>
__device__ __forceinline__ void scan_products(fr* lds, uint32_t count, In in, Out out) {
  const uint32_t tid = threadIdx.x, per = (count + GP_THREADS - 1u) / GP_THREADS, blocks = per ? (count + per - 1u) / per : 0u;
  const uint32_t lo = min(tid * per, count), hi = min(lo + per, count);
  fr blk = cg1fr::fr_one();
  for (uint32_t i = lo; i < hi; ++i) blk = cg1fr::fr_mul(blk, in(i));
  lds[tid] = blk;
  __syncthreads();
  for (uint32_t dd = 1u; dd < blocks; dd <<= 1) {
    fr t = lds[tid];
    if (tid >= dd) t = cg1fr::fr_mul(lds[tid - dd], t);
    __syncthreads();
    lds[tid] = t;
    __syncthreads();
  }
  fr pre = tid ? lds[tid - 1u] : cg1fr::fr_one();
  __syncthreads();
  for (uint32_t i = lo; i < hi; ++i) {
    out(i, pre);
    if (i + 1u < hi) pre = cg1fr::fr_mul(pre, in(i));
  }
}

// two sums over the workgroup at once (the tree of k_ipa_step): the totals in red[0][0], red[1][0] for every lane
__device__ __forceinline__ void tree_sum2(fr (*red)[GP_THREADS], const fr& x, const fr& y) {
  const uint32_t tid = threadIdx.x;
  red[0][tid] = x; red[1][tid] = y;
  __syncthreads();
  for (uint32_t dd = GP_THREADS / 2u; dd >= 1u; dd >>= 1) {
    if (tid < dd) {
      red[0][tid] = cg1fr::fr_add(red[0][tid], red[0][tid + dd]);
      red[1][tid] = cg1fr::fr_add(red[1][tid], red[1][tid + dd]);
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(GP_THREADS) k_gprod_step(GprodArgs a, uint32_t phase) {
  __shared__ cg1chain::StepLds s;
  __shared__ fr s_red[2][GP_THREADS];
  __shared__ fr s_x[5];                      // c[ell-1] b[ell-1] | r_p | beta^ell | beta^(ell+1) | beta^-(ell+1)

  const uint32_t tid = threadIdx.x, p = blockIdx.x, n = a.ipa.n0, ell = a.ell, nb = a.nb;
  const unsigned long long t_in = __builtin_amdgcn_s_memtime();
  const size_t vo = (size_t)p * n;
  cg1ipa::View v;
  v.c = a.ipa.c + vo; v.d = a.ipa.d + vo; v.kG = a.ipa.kG + vo; v.kGp = a.ipa.kGp + vo;
  v.gi = a.ipa.gi + vo; v.gpi = a.ipa.gpi + vo; v.hi = a.ipa.hi[p]; v.n0 = n;
  const uint64_t* vb = a.vb + 4u * vo;
  const uint64_t* r = a.ipa.rc + 4u * vo;
  uint64_t* z = a.z + 4u * vo;
  uint8_t* row = a.row + (size_t)p * GP_ROW;
  const uint64_t* gres = reinterpret_cast<const uint64_t*>(row + 48);

  if (phase == GP_BEGIN) {
    const uint64_t* cbl = a.cbl + 4u * (size_t)p * nb;
    scan_products(s_red[0], ell, [&](uint32_t i) { return load_le(vb + 4u * i); },
                  [&](uint32_t i, const fr& pre) {
                    v.c[i] = pre;
                    if (i == ell - 1u) s_x[0] = cg1fr::fr_mul(pre, load_le(vb + 4u * i));
                  });
    for (uint32_t k = tid; k < nb; k += GP_THREADS) v.c[ell + k] = load_le(cbl + 4u * k);
    __threadfence_block();
    __syncthreads();
    if (tid == 0u && !cg1fr::fr_eq(s_x[0], load_le(gres))) atomicOr(a.ipa.chain_status, ST_BAD_PRODUCT);
    uint32_t* tb = a.ipa.tb + (size_t)p * begin_terms(n);
    uint64_t* sc = a.ipa.sc + 4u * (size_t)p * begin_terms(n);
    for (uint32_t j = tid; j < n; j += GP_THREADS) begin_term(v.gi, n, j, load_le(vb + 4u * j), v.c[j], tb, sc);
    return;
  }

  // ---- the encodings of launch 1: B' against B, C into the proof and the two data rows; or (same_perm) A' against A, M' against M,
  // B' into the data row and the proof as B, then C, 12 words further on
  const uint32_t po = a.same_perm ? 12u : 0u;
  uint32_t* proof = a.proof + (size_t)p * a.proof_words;
  const uint32_t* pts = a.ipa.pts48 + (size_t)p * (a.same_perm ? 4u : 2u) * 12u;
  uint8_t* trow = a.ipa.trow + (size_t)p * cg1ipa::IPA_TROW;
  if (tid < 24u + 2u * po) {
    const uint32_t q = tid / 12u + (a.same_perm ? 0u : 2u), w = tid % 12u, val = pts[tid];      // q: A' | M' | B' | C
    if (q < 2u) {
      if (val != a.am48[(size_t)p * 24u + tid]) atomicOr(a.ipa.chain_status, q == 0u ? cg1sperm::ST_BAD_A : cg1sperm::ST_BAD_M);
    } else if (q == 2u) {
      if (a.same_perm) { reinterpret_cast<uint32_t*>(row)[w] = val; proof[w] = val; }
      else if (val != reinterpret_cast<const uint32_t*>(row)[w]) atomicOr(a.ipa.chain_status, ST_BAD_COMMITMENT);
    } else {
      proof[po + w] = val;
      reinterpret_cast<uint32_t*>(row + 80)[w] = val;
      reinterpret_cast<uint32_t*>(trow)[w] = val;
    }
  }
  // ---- gprod_step1 [B, gprod_result] -> gprod_alpha
  using cg1chain::label; using cg1chain::op;
  if (tid == 64u) {
    label(s.labels, "gprod_step1", 11); label(s.labels + 8, "gprod_alpha", 11); label(s.labels + 16, "gprod_step2", 11); label(s.labels + 24, "gprod_beta", 10);
    s.ops[0] = op(cg1merlin::OP_APPEND_POINT, 0, 11, 48, 0, 0);         // B
    s.ops[1] = op(cg1merlin::OP_APPEND, 0, 11, 32, 48, 0);              // gprod_result
    s.ops[2] = op(cg1merlin::OP_CHALLENGE_SCALAR, 1, 11, 32, 0, 0);     // alpha
  }
  uint32_t* ck = a.ipa.clocks ? a.ipa.clocks + 4u * p : nullptr;
  uint8_t* st = a.ipa.states + (size_t)p * 208;
  uint8_t* chal = a.ipa.chal + (size_t)p * 64;
  cg1chain::transcript_step(s, st, 3u, row, chal, a.ipa.msm_status, nullptr, a.ipa.chain_status, cg1chain::INV_NONE, nullptr, ck);
  const fr alpha = s.ch[0];
  // ---- r_p = <r_b + alpha, c_blinders>  (grand_prod.py:56-57)
  {
    fr acc = cg1fr::fr_zero();
    for (uint32_t k = tid; k < nb; k += GP_THREADS) acc = cg1fr::fr_add(acc, cg1fr::fr_mul(cg1fr::fr_add(load_le(vb + 4u * (ell + k)), alpha), v.c[ell + k]));
    tree_sum2(s_red, acc, acc);
    if (tid == 0u) {
      s_x[1] = s_red[0][0];
      cg1chain::put_scalar(proof + po + 12u, s_red[0][0]);
      cg1chain::put_scalar(reinterpret_cast<uint32_t*>(row + 128), s_red[0][0]);
    }
  }
  // ---- gprod_step2 [C, r_p] -> gprod_beta, then beta^-1
  if (tid == 64u) {
    s.ops[0] = op(cg1merlin::OP_APPEND_POINT, 2, 11, 48, 80, 0);        // C
    s.ops[1] = op(cg1merlin::OP_APPEND, 2, 11, 32, 128, 0);             // r_p
    s.ops[2] = op(cg1merlin::OP_CHALLENGE_SCALAR, 3, 10, 32, 0, 0);     // beta
  }
  cg1chain::transcript_step(s, st, 3u, row, chal, a.ipa.msm_status, nullptr, a.ipa.chain_status, cg1chain::INV_NONE, nullptr, ck);
  if (tid == 0u) {
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    if (cg1fr::fr_is_zero(s.ch[0])) { atomicOr(a.ipa.chain_status, ST_ZERO_BETA); s.ch[1] = cg1fr::fr_zero(); }
    else s.ch[1] = a.ipa.inv_fermat ? cg1chain::inv_fermat(s.ch[0]) : cg1chain::inv_binary(s.ch[0]);
    if (ck) ck[1] += (uint32_t)(__builtin_amdgcn_s_memtime() - t0);
  }
  __threadfence_block();
  __syncthreads();
  const fr beta = s.ch[0], beta_inv = s.ch[1];
  // ---- the powers of beta: d_j for j < ell, beta^ell, beta^(ell+1); those of beta^-1: kGp[j] = beta^-(j+1), beta^-(ell+1)
  scan_products(s_red[0], ell + 2u, [&](uint32_t) { return beta; },
                [&](uint32_t i, const fr& pw) {
                  if (i < ell) v.d[i] = d_elem(load_le(vb + 4u * i), beta, pw);
                  else s_x[2u + (i - ell)] = pw;
                });
  scan_products(s_red[0], ell + 2u, [&](uint32_t) { return beta_inv; },
                [&](uint32_t i, const fr& pw) {
                  if (i >= 1u && i <= ell) v.kGp[i - 1u] = pw;
                  if (i == ell + 1u) s_x[4] = pw;
                });
  __syncthreads();
  for (uint32_t k = tid; k < nb; k += GP_THREADS) {
    v.d[ell + k] = d_blinder(cg1fr::fr_add(load_le(vb + 4u * (ell + k)), alpha), s_x[3]);
    v.kGp[ell + k] = s_x[4];
  }
  for (uint32_t j = tid; j < n; j += GP_THREADS) v.kG[j] = cg1fr::fr_one();
  if (tid == 0u) cg1chain::put_scalar(reinterpret_cast<uint32_t*>(trow + 96), inner_prod(s_x[1], load_le(gres), s_x[2], s_x[3]));      // the IPA's z
  __threadfence_block();
  __syncthreads();
  // ---- generate_ipa_blinders after its draws: omega, delta, then the last two entries of z
  {
    fr so = cg1fr::fr_zero(), sd = cg1fr::fr_zero();
    for (uint32_t j = tid; j < n; j += GP_THREADS) {
      const fr rj = load_le(r + 4u * j);
      so = cg1fr::fr_add(so, cg1fr::fr_mul(rj, v.d[j]));
      if (j + 2u < n) {
        const fr zj = load_le(z + 4u * j);
        so = cg1fr::fr_add(so, cg1fr::fr_mul(zj, v.c[j]));
        sd = cg1fr::fr_add(sd, cg1fr::fr_mul(rj, zj));
      }
    }
    tree_sum2(s_red, so, sd);
    if (tid == 0u) {
      const unsigned long long t0 = __builtin_amdgcn_s_memtime();
      const fr r2 = load_le(r + 4u * (n - 2u)), r1 = load_le(r + 4u * (n - 1u)), c2 = v.c[n - 2u], c1 = v.c[n - 1u];
      const fr e = blinder_denominator(r2, r1, c2, c1);
      const uint32_t bad = (cg1fr::fr_is_zero(c2) ? ST_ZERO_C : 0u) | (cg1fr::fr_is_zero(e) ? ST_ZERO_DENOMINATOR : 0u);
      fr pen = cg1fr::fr_zero(), last = cg1fr::fr_zero();
      if (bad != 0u) atomicOr(a.ipa.chain_status, bad);
      else {
        const fr ec = cg1fr::fr_mul(e, c2);
        blinder_finish(s_red[0][0], s_red[1][0], r2, c2, c1, e, a.ipa.inv_fermat ? cg1chain::inv_fermat(ec) : cg1chain::inv_binary(ec), pen, last);
      }
      cg1fr::fr_to_le32(pen, reinterpret_cast<uint8_t*>(z + 4u * (n - 2u)));
      cg1fr::fr_to_le32(last, reinterpret_cast<uint8_t*>(z + 4u * (n - 1u)));
      if (ck) ck[1] += (uint32_t)(__builtin_amdgcn_s_memtime() - t0);
    }
  }
  __threadfence_block();
  __syncthreads();
  // ---- the terms of D, B_c, B_d
  uint32_t* tb = a.ipa.tb + (size_t)p * step_terms(n);
  uint64_t* sc = a.ipa.sc + 4u * (size_t)p * step_terms(n);
  for (uint32_t j = tid; j < n; j += GP_THREADS) {
    const fr bj = load_le(vb + 4u * j);
    step_term(v, j, j < ell ? cg1fr::fr_sub(bj, beta_inv) : cg1fr::fr_add(bj, alpha), load_le(r + 4u * j), load_le(z + 4u * j), tb, sc);
  }
  if (tid == 0u) cg1chain::step_clock(ck, t_in);
}

}  // namespace cg1gprod
