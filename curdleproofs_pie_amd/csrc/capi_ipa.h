// C ABI, part 9: the inner-product argument proved on the device (kernels_ipa.h over the tables of capi_fixed.h).
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

namespace {
struct IpaLayout {                           // byte offsets into the staging block (pinned host memory and its device twin: the same layout)
  size_t gi, gpi, hi, coef, vc, vd, rc, rd, trow, offs1, offsr;       // uploaded
  size_t status, clocks, states, proof;                               // uploaded (zeros | zeros | the callers' states | --) and read back
  size_t c, d, kG, kGp, kH, chal, pts, tb, sc;                        // device only
  size_t up_end, down_begin, down_end, total;
};
IpaLayout ipa_layout(size_t n, size_t P, size_t proof_bytes) {
  IpaLayout L{};
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 63) & ~(size_t)63; return at; };
  L.gi = take(P * n * 4); L.gpi = take(P * n * 4); L.hi = take(P * 4);
  L.coef = take(P * n * 32); L.vc = take(P * n * 32); L.vd = take(P * n * 32); L.rc = take(P * n * 32); L.rd = take(P * n * 32);
  L.trow = take(P * cg1ipa::IPA_TROW); L.offs1 = take((2 * P + 1) * 4); L.offsr = take((4 * P + 1) * 4);
  L.down_begin = o;
  L.status = take(16); L.clocks = take(P * 16); L.states = take(P * 208);
  L.up_end = o;
  L.proof = take(P * proof_bytes);
  L.down_end = o;
  L.c = take(P * n * 32); L.d = take(P * n * 32); L.kG = take(P * n * 32); L.kGp = take(P * n * 32); L.kH = take(P * 32);
  L.chal = take(P * 64); L.pts = take(P * 192);
  L.tb = take(P * (2 * n + 2) * 4); L.sc = take(P * (2 * n + 2) * 32);
  L.total = o;
  return L;
}
bool ipa_scalars_canonical(const uint8_t* s, size_t count) {
  for (size_t i = 0; i < count; ++i) {
    uint32_t w[8];
    memcpy(w, s + 32 * i, 32);
    if (!cg1::fixed_scalar_below_r(w)) return false;
  }
  return true;
}
}  // namespace

extern "C" {
size_t cg1_ipa_proof_bytes(size_t n) {
  if (n < 2 || (n & (n - 1)) != 0) return 0;
  size_t lg = 0;
  while (((size_t)1 << lg) < n) ++lg;
  return (2 + 4 * lg) * 48 + 64;
}

int cg1_ipa_prove_device(cg1_ctx* ctx, cg1_fixed* t, size_t n, size_t n_provers, const uint32_t* g_index, const uint32_t* g_prime_index,
                         const uint32_t* h_index, const uint8_t* g_prime_coeffs32, const uint8_t* cd48, const uint8_t* z32, const uint8_t* vec_c32,
                         const uint8_t* vec_d32, const uint8_t* vec_r_c32, const uint8_t* vec_r_d32, uint8_t* states208, uint8_t* out_proofs,
                         uint32_t* out_clocks) {
  if (!ctx) return CG1_ERR_HIP;
  if (n_provers == 0) return CG1_OK;
  // ---- refusals: the whole call, before anything is written
  if (!t || t->device != ctx->device || !g_index || !g_prime_index || !h_index || !cd48 || !z32 || !vec_c32 || !vec_d32 || !vec_r_c32 || !vec_r_d32 ||
      !states208 || !out_proofs) { snprintf(ctx->err, sizeof ctx->err, "cg1_ipa_prove_device: bad argument"); return CG1_ERR_ARG; }
  if (n < 2 || (n & (n - 1)) != 0 || n > CG1_IPA_MAX_N) {
    snprintf(ctx->err, sizeof ctx->err, "cg1_ipa_prove_device: n must be a power of two in 2 .. %d", CG1_IPA_MAX_N); return CG1_ERR_ARG; }
  if (n_provers > CG1_IPA_MAX_PROVERS) {
    snprintf(ctx->err, sizeof ctx->err, "cg1_ipa_prove_device: more than %d provers in one call", CG1_IPA_MAX_PROVERS); return CG1_ERR_ARG; }
  const size_t P = n_provers;
  for (size_t i = 0; i < P * n; ++i)
    if (g_index[i] >= t->n_bases || g_prime_index[i] >= t->n_bases) { snprintf(ctx->err, sizeof ctx->err, "cg1_ipa_prove_device: a base index is outside the table"); return CG1_ERR_ARG; }
  for (size_t i = 0; i < P; ++i)
    if (h_index[i] >= t->n_bases) { snprintf(ctx->err, sizeof ctx->err, "cg1_ipa_prove_device: a base index is outside the table"); return CG1_ERR_ARG; }
  if (!ipa_scalars_canonical(z32, P) || !ipa_scalars_canonical(vec_c32, P * n) || !ipa_scalars_canonical(vec_d32, P * n) ||
      !ipa_scalars_canonical(vec_r_c32, P * n) || !ipa_scalars_canonical(vec_r_d32, P * n) || (g_prime_coeffs32 && !ipa_scalars_canonical(g_prime_coeffs32, P * n))) {
    snprintf(ctx->err, sizeof ctx->err, "cg1_ipa_prove_device: a scalar is >= r: scalar32 must be a canonical Fr element"); return CG1_ERR_ENCODING; }
  for (size_t i = 0; i < 2 * P; ++i) {
    int inf = 0;
    const int rc = cg1_validate_compressed(cd48 + 48 * i, &inf);
    if (rc != CG1_OK) { snprintf(ctx->err, sizeof ctx->err, "cg1_ipa_prove_device: prover %zu: %s does not decode (status %d)", i / 2, (i & 1) ? "D" : "C", rc); return rc; }
  }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->pend.active = false;
  size_t lg = 0;
  while (((size_t)1 << lg) < n) ++lg;
  const size_t pb = cg1_ipa_proof_bytes(n);
  const IpaLayout L = ipa_layout(n, P, pb);
  { const int rc = cg1::grow_pinned_pair(ctx, t->h_ipa, nullptr, t->d_ipa, t->cap_ipa, L.total, L.total, hipHostMallocDefault); if (rc) return rc; }
  // ---- stage the inputs: one block, one copy
  uint8_t* H = t->h_ipa;
  uint8_t* D = t->d_ipa;
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
  memset(H + L.status, 0, 16); memset(H + L.clocks, 0, P * 16);
  memcpy(H + L.states, states208, P * 208);
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
  HIPCHK(hipMemcpyAsync(H + L.down_begin, D + L.down_begin, L.down_end - L.down_begin, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));                 // the one wait
  HIPCHK(hipGetLastError());
  { const int rc = table_status_error<FixedKind>(ctx, reinterpret_cast<const uint32_t*>(H + L.status)[0]); if (rc) return rc; }
  memcpy(out_proofs, H + L.proof, P * pb);
  memcpy(states208, H + L.states, P * 208);
  if (out_clocks) memcpy(out_clocks, H + L.clocks, P * 16);
  return CG1_OK;
}
}  // extern "C"
