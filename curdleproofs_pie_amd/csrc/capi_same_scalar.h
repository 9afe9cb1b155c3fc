// C ABI, part 14: the shuffle prover's same-scalar block proved on the device (kernels_same_scalar.h over ONE light table, built inside the
// call, of G_t | G_u | H | the provers' vec_R | vec_S -- the scratch capi_same_msm.h's chain keeps with the cg1_fixed handle).  The body is
// cut into check | stage | args | reserve | enqueue parts, which the whole-shuffle entry (capi_shuffle.h) runs inside its own pipeline.
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

static_assert(cg1sscalar::ST_NOT_G1 == CG1_SAME_SCALAR_NOT_G1 && CG1_SAME_SCALAR_NOT_G1 == 2 * CG1_SAME_PERM_BAD_M &&
              (CG1_SAME_SCALAR_NOT_G1 & (cg1gprod::ST_ALL | CG1_SAME_PERM_BAD_A | CG1_SAME_PERM_BAD_M)) == 0,
              "the header names the kernel's status bit, the next free one above the same-permutation argument's");
static_assert(cg1sscalar::MSMS * CG1_SAME_SCALAR_MAX_PROVERS <= CG1_LIGHT_MAX_MSMS && CG1_SAME_SCALAR_MAX_ELL + 1 <= CG1_LIGHT_MAX_TERMS, "one launch carries every prover's ten MSMs");

namespace {
struct SscalarLayout : ChainLayout {
  size_t bases96, va, k, bl, offs;                          // uploaded
  size_t chal, pts, tb, sc, in_g1;                          // device only
};
SscalarLayout sscalar_layout(size_t ell, size_t P, size_t base = 0, size_t states_at = ChainLayout::OWN_STATES) {
  SscalarLayout L{};
  L.begin(base);
  const size_t terms = cg1sscalar::terms((uint32_t)ell);
  L.bases96 = L.take((cg1sscalar::SHARED_BASES + P * 2 * ell) * 96); L.va = L.take(P * ell * 32); L.k = L.take(P * 32); L.bl = L.take(P * 5 * 32);
  L.offs = L.take((cg1sscalar::MSMS * P + 1) * 4);
  L.shared(P, cg1sscalar::PROOF_BYTES, states_at);
  L.chal = L.take(P * 32); L.pts = L.take(P * cg1sscalar::SS_ROW);
  L.tb = L.take(P * terms * 4); L.sc = L.take(P * terms * 32); L.in_g1 = L.take(P * 2 * ell);
  return L;
}
// the refusal the step kernel can only report
int same_scalar_status_error(cg1_ctx* ctx, const char* who, uint32_t st) {
  if (!(st & cg1sscalar::ST_NOT_G1)) return CG1_OK;
  snprintf(ctx->err, sizeof ctx->err, "%s: an entry of vec_R | vec_S is outside the prime-order subgroup G1 (R k and S k fold into the scalars only for bases of order r)", who);
  return CG1_ERR_NOT_IN_SUBGROUP;
}

// ---- refusals: the whole call, before anything is written.  vec_a32 null: an absent list (the whole-shuffle entry draws vec_a itself)
int sscalar_check(cg1_ctx* ctx, const char* who, const cg1_fixed* t, bool pointers_ok, size_t ell, size_t P, const uint8_t* gth_affine96, const uint8_t* rs_affine96,
                  const uint8_t* vec_a32, const uint8_t* k32, const uint8_t* blinders32) {
  static const char* const shared[] = {"crs_G_t", "crs_G_u", "crs_H"};
  if (!t || t->device != ctx->device || !pointers_ok) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", who); return CG1_ERR_ARG; }
  if (ell < 1 || ell > CG1_SAME_SCALAR_MAX_ELL) { snprintf(ctx->err, sizeof ctx->err, "%s: ell must be in 1 .. %d", who, CG1_SAME_SCALAR_MAX_ELL); return CG1_ERR_ARG; }
  if (P > CG1_SAME_SCALAR_MAX_PROVERS || cg1sscalar::SHARED_BASES + P * 2 * ell > CG1_LIGHT_MAX_BASES) {
    snprintf(ctx->err, sizeof ctx->err, "%s: more than %d provers, or more than %d bases G_t | G_u | H | R | S, in one call", who, CG1_SAME_SCALAR_MAX_PROVERS, CG1_LIGHT_MAX_BASES);
    return CG1_ERR_ARG; }
  if (const int rc = chain_check_scalars(ctx, who, {{vec_a32, P * ell}, {k32, P}, {blinders32, P * 5}})) return rc;
  const size_t n_bases = cg1sscalar::SHARED_BASES + P * 2 * ell;
  for (size_t b = 0; b < n_bases; ++b) {                    // canonical coordinates, on the curve (or the all-zero identity record)
    uint8_t blob[CG1_POINT_BYTES];
    const size_t e = b - cg1sscalar::SHARED_BASES;
    const int rc = cg1_from_affine96(blob, b < cg1sscalar::SHARED_BASES ? gth_affine96 + 96 * b : rs_affine96 + 96 * e, 1);
    if (rc == CG1_OK) continue;
    if (b < cg1sscalar::SHARED_BASES) snprintf(ctx->err, sizeof ctx->err, "%s: %s is not a curve point (status %d)", who, shared[b], rc);
    else snprintf(ctx->err, sizeof ctx->err, "%s: prover %zu: entry %zu of vec_R | vec_S is not a curve point (status %d)", who, e / (2 * ell), e % (2 * ell), rc);
    return rc;
  }
  return CG1_OK;
}
// ---- the inputs into the block (vec_a32 null: its field is filled by the caller; k32 and blinders32 null: a resident witness, placed on
// the device by k_whisk_witness_place)
void sscalar_stage(uint8_t* H, const SscalarLayout& L, size_t ell, size_t P, const uint8_t* gth_affine96, const uint8_t* rs_affine96, const uint8_t* vec_a32,
                   const uint8_t* k32, const uint8_t* blinders32) {
  const uint32_t el = (uint32_t)ell, Pn = (uint32_t)P, terms = cg1sscalar::terms(el);
  memcpy(H + L.bases96, gth_affine96, cg1sscalar::SHARED_BASES * 96);
  memcpy(H + L.bases96 + cg1sscalar::SHARED_BASES * 96, rs_affine96, P * 2 * ell * 96);
  if (vec_a32) memcpy(H + L.va, vec_a32, P * ell * 32);
  if (k32) { memcpy(H + L.k, k32, P * 32); memcpy(H + L.bl, blinders32, P * 5 * 32); }
  uint32_t* offs = reinterpret_cast<uint32_t*>(H + L.offs);
  for (uint32_t p = 0; p < Pn; ++p) cg1sscalar::offsets(el, p * terms, offs + cg1sscalar::MSMS * p);
}
cg1sscalar::SscalarArgs sscalar_args(uint8_t* D, const SscalarLayout& L, size_t ell, const cg1_light* lt, int bases_certified) {
  cg1sscalar::SscalarArgs a;
  a.ell = (uint32_t)ell;
  a.va = (const uint64_t*)(D + L.va); a.k = (const uint64_t*)(D + L.k); a.bl = (const uint64_t*)(D + L.bl);
  a.states = D + L.states; a.chal = D + L.chal;
  a.pts = (const uint32_t*)(D + L.pts); a.proof = (uint32_t*)(D + L.proof);
  a.tb = (uint32_t*)(D + L.tb); a.sc = (uint64_t*)(D + L.sc);
  a.in_g1 = bases_certified ? nullptr : D + L.in_g1;
  a.status_msm = lt->d_status; a.chain_status = (uint32_t*)(D + L.status); a.clocks = (uint32_t*)(D + L.clocks);
  return a;
}
// ---- the launch's shape and its slice sums, reserved BEFORE the first launch: table_enqueue would otherwise free and allocate in
// mid-chain, which waits for the device
int sscalar_reserve(cg1_ctx* ctx, cg1_light* lt, size_t ell, size_t P, TableShape& shape) {
  const uint32_t el = (uint32_t)ell, Pn = (uint32_t)P, M = cg1sscalar::MSMS * Pn, mt = el + 1u;
  shape = table_pick_shape<LightKind>(ctx, [&](uint32_t s) { return (size_t)Pn * (2u * ((el + s - 1) / s) + 4u * ((mt + s - 1) / s) + 4u); }, M, mt);
  const size_t Smax = (mt + shape.slice - 1) / shape.slice, need = Smax > 1 ? (size_t)M * Smax : 0;
  return cg1::grow_device(ctx, lt->d_partial, lt->cap_partial, need, need);
}
// ---- between the two phases of k_sscalar_step: build | [subgroup flags] | MSMs finish
int sscalar_enqueue_msms(cg1_ctx* ctx, cg1_light* lt, uint8_t* D, const SscalarLayout& L, const cg1sscalar::SscalarArgs& a, size_t ell, size_t P, int bases_certified,
                         TableShape shape) {
  const uint32_t el = (uint32_t)ell, Pn = (uint32_t)P, terms = cg1sscalar::terms(el), M = cg1sscalar::MSMS * Pn, mt = el + 1u;
  const size_t n_bases = cg1sscalar::SHARED_BASES + P * 2 * ell;
  light_build(ctx, D + L.bases96, n_bases, lt->d_tab);
  if (!bases_certified)
    hipLaunchKernelGGL(cg1::k_subgroup_row, dim3((unsigned)(P * 2 * ell)), dim3(64), 0, ctx->stream, (const uint32_t*)(D + L.bases96 + cg1sscalar::SHARED_BASES * 96),
                       (uint32_t)(P * 2 * ell), D + L.in_g1);
  return table_enqueue<LightKind>(ctx, lt, a.tb, (const uint32_t*)a.sc, (const uint32_t*)(D + L.offs), M, Pn * terms, mt, shape, false, nullptr, D + L.pts);
}
}  // namespace

extern "C" {
size_t cg1_same_scalar_proof_bytes(void) { return cg1sscalar::PROOF_BYTES; }

int cg1_same_scalar_prove_device(cg1_ctx* ctx, cg1_fixed* t, size_t ell, size_t n_provers, const uint8_t* gth_affine96, const uint8_t* rs_affine96,
                                 const uint8_t* vec_a32, const uint8_t* k32, const uint8_t* blinders32, int bases_certified, uint8_t* states208,
                                 uint8_t* out_proofs, uint32_t* out_clocks) {
  static const char* const who = "cg1_same_scalar_prove_device";
  if (!ctx) return CG1_ERR_HIP;
  if (n_provers == 0) return CG1_OK;
  const size_t P = n_provers;
  if (const int rc = sscalar_check(ctx, who, t, gth_affine96 && rs_affine96 && vec_a32 && k32 && blinders32 && states208 && out_proofs, ell, P, gth_affine96, rs_affine96,
                                   vec_a32, k32, blinders32)) return rc;
  const SscalarLayout L = sscalar_layout(ell, P);
  uint8_t* H; uint8_t* D;
  if (const int rc = chain_stage(ctx, t, L, P, states208, H, D)) return rc;
  cg1_light* lt;
  if (const int rc = chain_light_scratch(ctx, t, cg1sscalar::SHARED_BASES + P * 2 * ell, lt)) return rc;
  // ---- stage the inputs: one block, one copy
  sscalar_stage(H, L, ell, P, gth_affine96, rs_affine96, vec_a32, k32, blinders32);
  if (const int rc = chain_upload(ctx, t, L)) return rc;
  const cg1sscalar::SscalarArgs a = sscalar_args(D, L, ell, lt, bases_certified);
  TableShape shape;
  if (const int rc = sscalar_reserve(ctx, lt, ell, P, shape)) return rc;

  // ---- the chain: begin, build | [subgroup flags] | MSMs finish | step -- plain launches on the context's stream, no host wait between
  hipLaunchKernelGGL(cg1sscalar::k_sscalar_step, dim3((uint32_t)P), dim3(cg1sscalar::SS_THREADS), 0, ctx->stream, a, cg1sscalar::SS_BEGIN);
  if (const int rc = sscalar_enqueue_msms(ctx, lt, D, L, a, ell, P, bases_certified, shape)) return rc;
  hipLaunchKernelGGL(cg1sscalar::k_sscalar_step, dim3((uint32_t)P), dim3(cg1sscalar::SS_THREADS), 0, ctx->stream, a, cg1sscalar::SS_STEP);
  return chain_finish(ctx, t, L, P, cg1sscalar::PROOF_BYTES, states208, out_proofs, out_clocks, who, same_scalar_status_error);
}
}  // extern "C"
