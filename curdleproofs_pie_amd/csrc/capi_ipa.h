// C ABI, part 9: the inner-product argument proved on the device (kernels_ipa.h over the tables of capi_fixed.h).
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

namespace {
struct IpaLayout : ChainLayout {
  size_t gi, gpi, hi, coef, vc, vd, rc, rd, trow, offs1, offsr;       // uploaded
  size_t c, d, kG, kGp, kH, chal, pts, tb, sc;                        // device only
};
IpaLayout ipa_layout(size_t n, size_t P, size_t proof_bytes) {
  IpaLayout L{};
  L.gi = L.take(P * n * 4); L.gpi = L.take(P * n * 4); L.hi = L.take(P * 4);
  L.coef = L.take(P * n * 32); L.vc = L.take(P * n * 32); L.vd = L.take(P * n * 32); L.rc = L.take(P * n * 32); L.rd = L.take(P * n * 32);
  L.trow = L.take(P * cg1ipa::IPA_TROW); L.offs1 = L.take((2 * P + 1) * 4); L.offsr = L.take((4 * P + 1) * 4);
  L.shared(P, proof_bytes);
  L.c = L.take(P * n * 32); L.d = L.take(P * n * 32); L.kG = L.take(P * n * 32); L.kGp = L.take(P * n * 32); L.kH = L.take(P * 32);
  L.chal = L.take(P * 64); L.pts = L.take(P * 192);
  L.tb = L.take(P * (2 * n + 2) * 4); L.sc = L.take(P * (2 * n + 2) * 32);
  return L;
}
}  // namespace

extern "C" {
size_t cg1_ipa_proof_bytes(size_t n) { return chain_pow2(n) ? (2 + 4 * chain_lg(n)) * 48 + 64 : 0; }

int cg1_ipa_prove_device(cg1_ctx* ctx, cg1_fixed* t, size_t n, size_t n_provers, const uint32_t* g_index, const uint32_t* g_prime_index,
                         const uint32_t* h_index, const uint8_t* g_prime_coeffs32, const uint8_t* cd48, const uint8_t* z32, const uint8_t* vec_c32,
                         const uint8_t* vec_d32, const uint8_t* vec_r_c32, const uint8_t* vec_r_d32, uint8_t* states208, uint8_t* out_proofs,
                         uint32_t* out_clocks) {
  static const char* const who = "cg1_ipa_prove_device";
  static const char* const hashed[] = {"C", "D"};
  if (!ctx) return CG1_ERR_HIP;
  if (n_provers == 0) return CG1_OK;
  // ---- refusals: the whole call, before anything is written
  const size_t P = n_provers;
  if (const int rc = chain_check_shape(ctx, who, t, g_index && g_prime_index && h_index && cd48 && z32 && vec_c32 && vec_d32 && vec_r_c32 && vec_r_d32 &&
                                       states208 && out_proofs, n, CG1_IPA_MAX_N)) return rc;
  if (P > CG1_IPA_MAX_PROVERS) { snprintf(ctx->err, sizeof ctx->err, "%s: more than %d provers in one call", who, CG1_IPA_MAX_PROVERS); return CG1_ERR_ARG; }
  if (const int rc = chain_check_indices(ctx, who, t, {{g_index, P * n}, {g_prime_index, P * n}, {h_index, P}})) return rc;
  if (const int rc = chain_check_scalars(ctx, who, {{z32, P}, {vec_c32, P * n}, {vec_d32, P * n}, {vec_r_c32, P * n}, {vec_r_d32, P * n}, {g_prime_coeffs32, P * n}})) return rc;
  if (const int rc = chain_check_points(ctx, who, cd48, P, 2, hashed, nullptr)) return rc;
  const size_t lg = chain_lg(n), pb = cg1_ipa_proof_bytes(n);
  const IpaLayout L = ipa_layout(n, P, pb);
  // ---- stage the inputs: one block, one copy
  uint8_t* H; uint8_t* D;
  if (const int rc = chain_stage(ctx, t, L, P, states208, H, D)) return rc;
  memcpy(H + L.gi, g_index, P * n * 4); memcpy(H + L.gpi, g_prime_index, P * n * 4); memcpy(H + L.hi, h_index, P * 4);
  if (g_prime_coeffs32) memcpy(H + L.coef, g_prime_coeffs32, P * n * 32);
  memcpy(H + L.vc, vec_c32, P * n * 32); memcpy(H + L.vd, vec_d32, P * n * 32);
  memcpy(H + L.rc, vec_r_c32, P * n * 32); memcpy(H + L.rd, vec_r_d32, P * n * 32);
  uint32_t* offs1 = reinterpret_cast<uint32_t*>(H + L.offs1);
  uint32_t* offsr = reinterpret_cast<uint32_t*>(H + L.offsr);
  for (size_t p = 0; p < P; ++p) {
    uint8_t* row = H + L.trow + p * cg1ipa::IPA_TROW;
    memset(row, 0, cg1ipa::IPA_TROW);
    memcpy(row, cd48 + 96 * p, 96);
    memcpy(row + 96, z32 + 32 * p, 32);
    cg1ipa::step1_offsets((uint32_t)n, (uint32_t)(p * cg1ipa::step1_terms((uint32_t)n)), offs1 + 2 * p);
    cg1ipa::round_offsets((uint32_t)n, (uint32_t)(p * cg1ipa::round_terms((uint32_t)n)), offsr + 4 * p);
  }
  HIPCHK(hipMemcpyAsync(D, H, L.up_end, hipMemcpyHostToDevice, ctx->stream));

  cg1ipa::IpaArgs a;
  a.n0 = (uint32_t)n; a.lg = (uint32_t)lg; a.has_coeffs = g_prime_coeffs32 ? 1u : 0u; a.inv_fermat = ctx->ipa_inv ? 1u : 0u;
  a.gi = (const uint32_t*)(D + L.gi); a.gpi = (const uint32_t*)(D + L.gpi); a.hi = (const uint32_t*)(D + L.hi);
  a.coef = (const uint64_t*)(D + L.coef); a.vc = (const uint64_t*)(D + L.vc); a.vd = (const uint64_t*)(D + L.vd);
  a.rc = (const uint64_t*)(D + L.rc); a.rd = (const uint64_t*)(D + L.rd);
  a.c = (cg1fr::fr*)(D + L.c); a.d = (cg1fr::fr*)(D + L.d); a.kG = (cg1fr::fr*)(D + L.kG); a.kGp = (cg1fr::fr*)(D + L.kGp); a.kH = (cg1fr::fr*)(D + L.kH);
  a.states = D + L.states; a.trow = D + L.trow; a.chal = D + L.chal; a.pts48 = (const uint32_t*)(D + L.pts);
  a.proof = (uint32_t*)(D + L.proof); a.proof_words = (uint32_t)(pb / 4);
  a.tb = (uint32_t*)(D + L.tb); a.sc = (uint64_t*)(D + L.sc);
  a.msm_status = t->d_status; a.chain_status = (uint32_t*)(D + L.status); a.clocks = (uint32_t*)(D + L.clocks);

  // ---- the chain: begin | MSM finish step1 | (MSM finish round) x lg n -- plain launches on the context's stream, no host wait between
  const uint32_t Pn = (uint32_t)P, nn = (uint32_t)n;
  hipLaunchKernelGGL(cg1ipa::k_ipa_step, dim3(Pn), dim3(cg1ipa::IPA_THREADS), 0, ctx->stream, a, cg1ipa::IPA_BEGIN, nn, 0u);
  {
    const uint32_t M = 2 * Pn;
    const int rc = table_enqueue<FixedKind>(ctx, t, a.tb, (const uint32_t*)a.sc, (const uint32_t*)(D + L.offs1), M, Pn * cg1ipa::step1_terms(nn), nn, table_pick_shape<FixedKind>(ctx, M, nn), false, nullptr, D + L.pts);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(cg1ipa::k_ipa_step, dim3(Pn), dim3(cg1ipa::IPA_THREADS), 0, ctx->stream, a, cg1ipa::IPA_STEP1, nn, 0u);
  for (uint32_t r = 0; r < (uint32_t)lg; ++r) {
    const uint32_t M = 4 * Pn, mt = nn / 2 + 1;
    const int rc = table_enqueue<FixedKind>(ctx, t, a.tb, (const uint32_t*)a.sc, (const uint32_t*)(D + L.offsr), M, Pn * cg1ipa::round_terms(nn), mt, table_pick_shape<FixedKind>(ctx, M, mt), false, nullptr, D + L.pts);
    if (rc) return rc;
    hipLaunchKernelGGL(cg1ipa::k_ipa_step, dim3(Pn), dim3(cg1ipa::IPA_THREADS), 0, ctx->stream, a, cg1ipa::IPA_ROUND, nn >> r, r);
  }
  return chain_finish(ctx, t, L, P, pb, states208, out_proofs, out_clocks);
}
}  // extern "C"
