// C ABI, part 12: the grand-product argument proved on the device (kernels_gprod.h, then the phases of kernels_ipa.h, over the tables of
// capi_fixed.h).  Its body, gprod_chain, also carries the same-permutation argument (capi_same_perm.h: another head, the same chain); it
// is cut into check | plan | stage | head | args | reserve | enqueue parts, which the whole-shuffle entry (capi_shuffle.h) runs inside
// its own pipeline.
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

static_assert(cg1gprod::ST_BAD_COMMITMENT == CG1_GPROD_BAD_COMMITMENT && cg1gprod::ST_BAD_PRODUCT == CG1_GPROD_BAD_PRODUCT && cg1gprod::ST_ZERO_BETA == CG1_GPROD_ZERO_BETA &&
              cg1gprod::ST_ZERO_C == CG1_GPROD_ZERO_C && cg1gprod::ST_ZERO_DENOMINATOR == CG1_GPROD_ZERO_DENOMINATOR, "the header names the kernel's status bits");

namespace {
struct GprodLayout : ChainLayout {
  size_t gi, ui, vb, cbl, r, z, row, offs_b, offs_s, offsr;           // uploaded (z: the step kernel completes its last two entries)
  size_t va, perm, abl, mbl, am, ab;                                  // uploaded, the same-permutation head only (vb is then device only)
  size_t c, d, kG, kGp, kH, trow, chal, pts, tb, sc;                  // device only
};
// per0: the MSMs per prover of the first launch -- 2 (B' | C), or 4 with the same-permutation head (A' | M' | B' | C)
GprodLayout gprod_layout(size_t ell, size_t nb, size_t P, size_t proof_bytes, size_t per0, size_t base = 0, size_t states_at = ChainLayout::OWN_STATES) {
  GprodLayout L{};
  L.begin(base);
  const size_t n = ell + nb;
  const bool sp = per0 == 4;
  L.gi = L.take(P * n * 4); L.ui = L.take(P * 4);
  if (!sp) L.vb = L.take(P * n * 32);
  L.cbl = L.take(P * nb * 32); L.r = L.take(P * n * 32); L.z = L.take(P * n * 32);
  L.row = L.take(P * cg1gprod::GP_ROW); L.offs_b = L.take((per0 * P + 1) * 4); L.offs_s = L.take((3 * P + 1) * 4); L.offsr = L.take((4 * P + 1) * 4);
  if (sp) {
    L.va = L.take(P * ell * 32); L.perm = L.take(P * ell * 4); L.abl = L.take(P * nb * 32); L.mbl = L.take(P * nb * 32);
    L.am = L.take(P * 96); L.ab = L.take(P * 64);
  }
  L.shared(P, proof_bytes, states_at);
  if (sp) L.vb = L.take(P * n * 32);
  L.c = L.take(P * n * 32); L.d = L.take(P * n * 32); L.kG = L.take(P * n * 32); L.kGp = L.take(P * n * 32); L.kH = L.take(P * 32);
  L.trow = L.take(P * cg1ipa::IPA_TROW); L.chal = L.take(P * 64); L.pts = L.take(P * 192);                 // 4 encodings per prover
  const size_t terms = std::max<size_t>(3, per0) * n;                  // 3 n >= the rounds' 2 n + 2
  L.tb = L.take(P * terms * 4); L.sc = L.take(P * terms * 32);
  return L;
}
// the refusals the step kernel can only report: each with its own text
const char* gprod_status_text(uint32_t st) {
  const char* what = nullptr;
  if (st & cg1gprod::ST_BAD_PRODUCT) what = "gprod_result is not the product of vec_b";
  else if (st & cg1gprod::ST_BAD_COMMITMENT) what = "B is not the commitment MSM(crs_G_vec | crs_H_vec, vec_b | vec_b_blinders)";
  else if (st & cg1gprod::ST_ZERO_BETA) what = "the challenge gprod_beta is zero";
  else if (st & cg1gprod::ST_ZERO_C) what = "vec_c_blinders[n_blinders - 2] is zero: generate_ipa_blinders divides by it";
  else if (st & cg1gprod::ST_ZERO_DENOMINATOR) what = "the second denominator of generate_ipa_blinders is zero: draw ipa_r again";
  return what;
}
int gprod_status_error(cg1_ctx* ctx, const char* who, uint32_t st) {
  const char* what = gprod_status_text(st);
  if (!what) return CG1_OK;
  snprintf(ctx->err, sizeof ctx->err, "%s: %s", who, what);
  return CG1_ERR_ARG;
}

// What the same-permutation argument puts in front of the chain (capi_same_perm.h); null for the grand-product argument itself, whose
// B, gprod_result and vec_b are then the caller's.
struct SamePermHead {
  const uint8_t* am48;                       // [P][2][48]: A, M
  const uint8_t* vec_a32;                    // [P][ell]
  const uint32_t* perm;                      // [P][ell]
  const uint8_t* vec_a_blinders32;           // [P][nb]
  const uint8_t* vec_m_blinders32;           // [P][nb]
};

// The shape of one call of the chain: what its parts share.
struct GprodPlan {
  size_t ell, nb, n, P, lg, pb;
  uint32_t per0, po;                         // the first launch's MSMs per prover; B's 12 words in front of the proof
  GprodLayout L;
  TableShape shape[3];
};
GprodPlan gprod_plan(size_t ell, size_t nb, size_t P, bool sp, size_t base = 0, size_t states_at = ChainLayout::OWN_STATES) {
  GprodPlan g{};
  g.ell = ell; g.nb = nb; g.n = ell + nb; g.P = P; g.lg = chain_lg(g.n);
  g.pb = cg1_gprod_proof_bytes(ell, nb) + (sp ? 48 : 0);
  g.per0 = sp ? 4u : 2u; g.po = sp ? 12u : 0u;
  g.L = gprod_layout(ell, nb, P, g.pb, g.per0, base, states_at);
  return g;
}

// ---- refusals: the whole call, before anything is written.  sp == nullptr: the grand-product argument as the caller states it
// (gprod_result32, vec_b32).  hashed48: the `per` points per prover a transcript only hashes (B; A, M), named `names`; canon: a copy as
// the transcript absorbs them.  A null scalar list is an absent one (the whole-shuffle entry draws vec_a itself and forms A on the device).
int gprod_check(cg1_ctx* ctx, const char* who, ChainOwnStatus own_status, const cg1_fixed* t, bool pointers_ok, size_t ell, size_t nb, size_t P, const uint32_t* g_index,
                const uint32_t* u_index, const SamePermHead* sp, const uint8_t* hashed48, size_t per, const char* const* names, uint8_t* canon,
                const uint8_t* gprod_result32, const uint8_t* vec_b32, const uint8_t* vec_c_blinders32, const uint8_t* ipa_r32, const uint8_t* ipa_z_head32) {
  const size_t n = ell + nb;
  if (const int rc = chain_check_shape(ctx, who, t, pointers_ok && n >= ell, n, CG1_IPA_MAX_N)) return rc;
  if (ell < 1 || nb < 2) { snprintf(ctx->err, sizeof ctx->err, "%s: ell >= 1 and n_blinders >= 2", who); return CG1_ERR_ARG; }
  if (P > CG1_IPA_MAX_PROVERS) { snprintf(ctx->err, sizeof ctx->err, "%s: more than %d provers in one call", who, CG1_IPA_MAX_PROVERS); return CG1_ERR_ARG; }
  if (const int rc = chain_check_indices(ctx, who, t, {{g_index, P * n}, {u_index, P}})) return rc;
  if (sp) {
    for (size_t i = 0; sp->perm && i < P * ell; ++i)        // the kernel gathers vec_a[perm[i]]; the reference's get_permutation raises IndexError
      if (sp->perm[i] >= ell) { snprintf(ctx->err, sizeof ctx->err, "%s: a permutation entry is >= ell", who); return CG1_ERR_ARG; }
    if (const int rc = chain_check_scalars(ctx, who, {{sp->vec_a32, P * ell}, {sp->vec_a_blinders32, P * nb}, {sp->vec_m_blinders32, P * nb}, {vec_c_blinders32, P * nb},
                                                      {ipa_r32, P * n}, {ipa_z_head32, P * (n - 2)}})) return rc;
  } else {
    if (const int rc = chain_check_scalars(ctx, who, {{gprod_result32, P}, {vec_b32, P * n}, {vec_c_blinders32, P * nb}, {ipa_r32, P * n}, {ipa_z_head32, P * (n - 2)}})) return rc;
  }
  if (const int rc = chain_check_points(ctx, who, hashed48, P, per, names, canon)) return rc;
  for (size_t p = 0; vec_c_blinders32 && p < P; ++p) {      // c[n-2], the first denominator of generate_ipa_blinders (ipa.py:36)
    static const uint8_t zero[32] = {0};
    if (memcmp(vec_c_blinders32 + 32 * (p * nb + nb - 2), zero, 32) == 0) return own_status(ctx, who, cg1gprod::ST_ZERO_C);
  }
  return CG1_OK;
}
// ---- the inputs into the block, but for the same-permutation head's vec_a, A | M and challenges (same_perm_head).  canon_b: B as the
// transcript absorbs it (the grand-product argument only).  A null witness list (vec_c_blinders32, ipa_r32, ipa_z_head32, sp's perm and
// blinders): its field is not written here -- a resident witness, placed on the device (k_whisk_witness_place)
void gprod_stage(uint8_t* H, const GprodPlan& g, const uint32_t* g_index, const uint32_t* u_index, const SamePermHead* sp, const uint8_t* canon_b,
                 const uint8_t* gprod_result32, const uint8_t* vec_b32, const uint8_t* vec_c_blinders32, const uint8_t* ipa_r32, const uint8_t* ipa_z_head32) {
  const GprodLayout& L = g.L;
  const size_t P = g.P, n = g.n, nb = g.nb, ell = g.ell;
  memcpy(H + L.gi, g_index, P * n * 4); memcpy(H + L.ui, u_index, P * 4);
  if (!sp) memcpy(H + L.vb, vec_b32, P * n * 32);
  if (vec_c_blinders32) memcpy(H + L.cbl, vec_c_blinders32, P * nb * 32);
  if (ipa_r32) memcpy(H + L.r, ipa_r32, P * n * 32);
  const uint32_t nn = (uint32_t)n;
  uint32_t* offs_b = reinterpret_cast<uint32_t*>(H + L.offs_b);
  uint32_t* offs_s = reinterpret_cast<uint32_t*>(H + L.offs_s);
  uint32_t* offsr = reinterpret_cast<uint32_t*>(H + L.offsr);
  for (size_t p = 0; p < P; ++p) {
    uint8_t* row = H + L.row + p * cg1gprod::GP_ROW;
    memset(row, 0, cg1gprod::GP_ROW);
    if (!sp) {
      memcpy(row, canon_b + 48 * p, 48);
      memcpy(row + 48, gprod_result32 + 32 * p, 32);
    }
    if (ipa_z_head32) {
      uint8_t* z = H + L.z + p * n * 32;
      memcpy(z, ipa_z_head32 + p * (n - 2) * 32, (n - 2) * 32);
      memset(z + (n - 2) * 32, 0, 64);
    }
    if (sp) cg1sperm::begin_offsets(nn, (uint32_t)(p * cg1sperm::begin_terms(nn)), offs_b + 4 * p);
    else cg1gprod::begin_offsets(nn, (uint32_t)(p * cg1gprod::begin_terms(nn)), offs_b + 2 * p);
    cg1gprod::step_offsets(nn, (uint32_t)(p * cg1gprod::step_terms(nn)), offs_s + 3 * p);
    cg1ipa::round_offsets(nn, (uint32_t)(p * cg1ipa::round_terms(nn)), offsr + 4 * p);
  }
  if (sp && sp->perm) {
    memcpy(H + L.perm, sp->perm, P * ell * 4);
    memcpy(H + L.abl, sp->vec_a_blinders32, P * nb * 32); memcpy(H + L.mbl, sp->vec_m_blinders32, P * nb * 32);
  }
}
// The same-permutation head of prover p: same_perm_step1 [A, M], same_perm_step1 vec_a and the two challenges depend on nothing the
// chain computes (~25 Keccak permutations at ell = 124): run on the host, on the state that goes up.  am96: A | M as absorbed.
void same_perm_head(uint8_t* H, const GprodPlan& g, size_t p, const uint8_t* am96, const uint8_t* vec_a32) {
  static const uint8_t step1[] = "same_perm_step1", l_alpha[] = "same_perm_alpha", l_beta[] = "same_perm_beta";
  const GprodLayout& L = g.L;
  memcpy(H + L.va + p * g.ell * 32, vec_a32, g.ell * 32);
  memcpy(H + L.am + 96 * p, am96, 96);
  uint8_t* st = H + L.states + 208 * p;
  cg1_merlin_append_list(st, step1, 15, am96, 48, 2);
  cg1_merlin_append_list(st, step1, 15, vec_a32, 32, g.ell);
  cg1_merlin_challenge_scalar(st, l_alpha, 15, H + L.ab + 64 * p);
  cg1_merlin_challenge_scalar(st, l_beta, 14, H + L.ab + 64 * p + 32);
}
cg1sperm::SamePermArgs gprod_args(const cg1_ctx* ctx, const cg1_fixed* t, uint8_t* D, const GprodPlan& g, bool sp) {
  const GprodLayout& L = g.L;
  cg1sperm::SamePermArgs sa;
  cg1gprod::GprodArgs& a = sa.g;
  cg1ipa::IpaArgs& ia = a.ipa;
  ia.n0 = (uint32_t)g.n; ia.lg = (uint32_t)g.lg; ia.has_coeffs = 1u; ia.inv_fermat = ctx->ipa_inv ? 1u : 0u; ia.d_first = 1u;
  ia.gi = (const uint32_t*)(D + L.gi); ia.gpi = ia.gi; ia.hi = (const uint32_t*)(D + L.ui);
  ia.coef = nullptr; ia.vc = nullptr; ia.vd = nullptr;       // the IPA's begin phase is not launched: k_gprod_step leaves its state
  ia.rc = (const uint64_t*)(D + L.r); ia.rd = (const uint64_t*)(D + L.z);
  ia.c = (cg1fr::fr*)(D + L.c); ia.d = (cg1fr::fr*)(D + L.d); ia.kG = (cg1fr::fr*)(D + L.kG); ia.kGp = (cg1fr::fr*)(D + L.kGp); ia.kH = (cg1fr::fr*)(D + L.kH);
  ia.states = D + L.states; ia.trow = D + L.trow; ia.chal = D + L.chal; ia.pts48 = (const uint32_t*)(D + L.pts);
  ia.proof = (uint32_t*)(D + L.proof) + g.po + 20; ia.proof_words = (uint32_t)(g.pb / 4);       // behind [B |] C | r_p
  ia.tb = (uint32_t*)(D + L.tb); ia.sc = (uint64_t*)(D + L.sc);
  ia.msm_status = t->d_status; ia.chain_status = (uint32_t*)(D + L.status); ia.clocks = (uint32_t*)(D + L.clocks);
  a.ell = (uint32_t)g.ell; a.nb = (uint32_t)g.nb;
  a.vb = (const uint64_t*)(D + L.vb); a.cbl = (const uint64_t*)(D + L.cbl); a.z = (uint64_t*)(D + L.z);
  a.row = D + L.row; a.proof = (uint32_t*)(D + L.proof); a.proof_words = (uint32_t)(g.pb / 4);
  if (sp) {
    a.same_perm = 1u; a.am48 = (const uint32_t*)(D + L.am);
    sa.va = (const uint64_t*)(D + L.va); sa.perm = (const uint32_t*)(D + L.perm);
    sa.abl = (const uint64_t*)(D + L.abl); sa.mbl = (const uint64_t*)(D + L.mbl);
    sa.ab = (const uint64_t*)(D + L.ab); sa.vb = (uint64_t*)(D + L.vb);
  }
  return sa;
}
// ---- the launches' shapes, and the slice sums of the largest of them reserved BEFORE the first launch: table_enqueue would otherwise
// free and allocate in mid-chain, which waits for the device
int gprod_reserve(cg1_ctx* ctx, cg1_fixed* t, GprodPlan& g) {
  const uint32_t Pn = (uint32_t)g.P, nn = (uint32_t)g.n;
  const uint32_t per[3] = {g.per0, 3, 4}, mts[3] = {nn, nn, nn / 2 + 1};
  size_t need = 0;
  for (int k = 0; k < 3; ++k) {
    g.shape[k] = table_pick_shape<FixedKind>(ctx, per[k] * Pn, mts[k]);
    const size_t S = (mts[k] + g.shape[k].slice - 1) / g.shape[k].slice;
    if (S > 1) need = std::max(need, (size_t)per[k] * Pn * S);
  }
  return cg1::grow_device(ctx, t->d_partial, t->cap_partial, need, need);
}
// ---- the chain: begin | MSM finish step | MSM finish, the IPA's step1 | (MSM finish round) x lg n -- plain launches on the context's
// stream, no host wait between
int gprod_enqueue(cg1_ctx* ctx, cg1_fixed* t, uint8_t* D, const GprodPlan& g, const cg1sperm::SamePermArgs& sa, bool sp) {
  const GprodLayout& L = g.L;
  const cg1gprod::GprodArgs& a = sa.g;
  const cg1ipa::IpaArgs& ia = a.ipa;
  const uint32_t Pn = (uint32_t)g.P, nn = (uint32_t)g.n;
  const uint32_t per[3] = {g.per0, 3, 4}, mts[3] = {nn, nn, nn / 2 + 1};
  auto msms = [&](int k, size_t offs, uint32_t n_terms) {
    return table_enqueue<FixedKind>(ctx, t, ia.tb, (const uint32_t*)ia.sc, (const uint32_t*)(D + offs), per[k] * Pn, n_terms, mts[k], g.shape[k], false, nullptr, D + L.pts);
  };
  if (sp) hipLaunchKernelGGL(cg1sperm::k_same_perm_begin, dim3(Pn), dim3(cg1gprod::GP_THREADS), 0, ctx->stream, sa);
  else hipLaunchKernelGGL(cg1gprod::k_gprod_step, dim3(Pn), dim3(cg1gprod::GP_THREADS), 0, ctx->stream, a, cg1gprod::GP_BEGIN);
  if (const int rc = msms(0, L.offs_b, Pn * g.per0 * nn)) return rc;
  hipLaunchKernelGGL(cg1gprod::k_gprod_step, dim3(Pn), dim3(cg1gprod::GP_THREADS), 0, ctx->stream, a, cg1gprod::GP_STEP);
  if (const int rc = msms(1, L.offs_s, Pn * cg1gprod::step_terms(nn))) return rc;
  hipLaunchKernelGGL(cg1ipa::k_ipa_step, dim3(Pn), dim3(cg1ipa::IPA_THREADS), 0, ctx->stream, ia, cg1ipa::IPA_STEP1, nn, 0u);
  for (uint32_t r = 0; r < (uint32_t)g.lg; ++r) {
    if (const int rc = msms(2, L.offsr, Pn * cg1ipa::round_terms(nn))) return rc;
    hipLaunchKernelGGL(cg1ipa::k_ipa_step, dim3(Pn), dim3(cg1ipa::IPA_THREADS), 0, ctx->stream, ia, cg1ipa::IPA_ROUND, nn >> r, r);
  }
  return CG1_OK;
}

// The chain of both arguments.  who / own_status: the entry's name and its status texts.  sp == nullptr: the grand-product argument as
// the caller states it (b48, gprod_result32, vec_b32).  Otherwise those three are null: the host runs the transcript head on the staged
// states, k_same_perm_begin forms vec_b and gprod_result on the device, and the step phase checks A and M and emits B.
int gprod_chain(cg1_ctx* ctx, cg1_fixed* t, const char* who, ChainOwnStatus own_status, size_t ell, size_t n_blinders, size_t n_provers,
                const uint32_t* g_index, const uint32_t* u_index, const SamePermHead* sp, const uint8_t* b48, const uint8_t* gprod_result32, const uint8_t* vec_b32,
                const uint8_t* vec_c_blinders32, const uint8_t* ipa_r32, const uint8_t* ipa_z_head32, uint8_t* states208, uint8_t* out_proofs, uint32_t* out_clocks) {
  static const char* const hashed_b[] = {"B"};
  static const char* const hashed_am[] = {"A", "M"};
  if (!ctx) return CG1_ERR_HIP;
  if (n_provers == 0) return CG1_OK;
  const size_t P = n_provers;
  const bool own_ok = sp ? sp->am48 && sp->vec_a32 && sp->perm && sp->vec_a_blinders32 && sp->vec_m_blinders32 : b48 && gprod_result32 && vec_b32;
  std::vector<uint8_t> canon(P * (sp ? 96 : 48));
  if (const int rc = gprod_check(ctx, who, own_status, t, g_index && u_index && own_ok && vec_c_blinders32 && ipa_r32 && ipa_z_head32 && states208 && out_proofs,
                                 ell, n_blinders, P, g_index, u_index, sp, sp ? sp->am48 : b48, sp ? 2 : 1, sp ? hashed_am : hashed_b, canon.data(),
                                 gprod_result32, vec_b32, vec_c_blinders32, ipa_r32, ipa_z_head32)) return rc;
  GprodPlan g = gprod_plan(ell, n_blinders, P, sp != nullptr);
  // ---- stage the inputs: one block, one copy
  uint8_t* H; uint8_t* D;
  if (const int rc = chain_stage(ctx, t, g.L, P, states208, H, D)) return rc;
  gprod_stage(H, g, g_index, u_index, sp, canon.data(), gprod_result32, vec_b32, vec_c_blinders32, ipa_r32, ipa_z_head32);
  if (sp)                                                   // the caller's states are written by chain_finish alone
    for (size_t p = 0; p < P; ++p) same_perm_head(H, g, p, &canon[96 * p], sp->vec_a32 + p * ell * 32);
  if (const int rc = chain_upload(ctx, t, g.L)) return rc;
  const cg1sperm::SamePermArgs sa = gprod_args(ctx, t, D, g, sp != nullptr);
  if (const int rc = gprod_reserve(ctx, t, g)) return rc;
  if (const int rc = gprod_enqueue(ctx, t, D, g, sa, sp != nullptr)) return rc;
  return chain_finish(ctx, t, g.L, P, g.pb, states208, out_proofs, out_clocks, who, own_status);
}
}  // namespace

extern "C" {
size_t cg1_gprod_proof_bytes(size_t ell, size_t n_blinders) {
  const size_t n = ell + n_blinders;
  return ell >= 1 && n_blinders >= 2 && n > ell && chain_pow2(n) ? 48 + 32 + cg1_ipa_proof_bytes(n) : 0;
}

int cg1_gprod_prove_device(cg1_ctx* ctx, cg1_fixed* t, size_t ell, size_t n_blinders, size_t n_provers, const uint32_t* g_index, const uint32_t* u_index,
                           const uint8_t* b48, const uint8_t* gprod_result32, const uint8_t* vec_b32, const uint8_t* vec_c_blinders32, const uint8_t* ipa_r32,
                           const uint8_t* ipa_z_head32, uint8_t* states208, uint8_t* out_proofs, uint32_t* out_clocks) {
  return gprod_chain(ctx, t, "cg1_gprod_prove_device", gprod_status_error, ell, n_blinders, n_provers, g_index, u_index, nullptr, b48, gprod_result32, vec_b32,
                     vec_c_blinders32, ipa_r32, ipa_z_head32, states208, out_proofs, out_clocks);
}
}  // extern "C"
