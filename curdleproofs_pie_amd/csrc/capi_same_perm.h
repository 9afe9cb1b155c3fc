// C ABI, part 13: the same-permutation argument proved on the device -- the grand-product chain of capi_gprod.h (gprod_chain) with the
// host transcript head and k_same_perm_begin (kernels_same_perm.h) in front of it.
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

static_assert(cg1sperm::ST_BAD_A == CG1_SAME_PERM_BAD_A && cg1sperm::ST_BAD_M == CG1_SAME_PERM_BAD_M && (cg1gprod::ST_ALL & (CG1_SAME_PERM_BAD_A | CG1_SAME_PERM_BAD_M)) == 0,
              "the header names the kernel's status bits, above the grand-product argument's");

namespace {
// the refusals the step kernel can only report: the two of this argument, then the grand-product chain's own
int same_perm_status_error(cg1_ctx* ctx, const char* who, uint32_t st) {
  const char* what = nullptr;
  if (st & cg1sperm::ST_BAD_A) what = "A is not the commitment MSM(crs_G_vec | crs_H_vec, vec_a∘permutation | vec_a_blinders)";
  else if (st & cg1sperm::ST_BAD_M) what = "M is not the commitment MSM(crs_G_vec | crs_H_vec, permutation | vec_m_blinders)";
  else what = gprod_status_text(st);
  if (!what) return CG1_OK;
  snprintf(ctx->err, sizeof ctx->err, "%s: %s", who, what);
  return CG1_ERR_ARG;
}
}  // namespace

extern "C" {
size_t cg1_same_perm_proof_bytes(size_t ell, size_t n_blinders) {
  const size_t pb = cg1_gprod_proof_bytes(ell, n_blinders);
  return pb ? 48 + pb : 0;
}

int cg1_same_perm_prove_device(cg1_ctx* ctx, cg1_fixed* t, size_t ell, size_t n_blinders, size_t n_provers, const uint32_t* g_index, const uint32_t* u_index,
                               const uint8_t* am48, const uint8_t* vec_a32, const uint32_t* perm, const uint8_t* vec_a_blinders32, const uint8_t* vec_m_blinders32,
                               const uint8_t* vec_c_blinders32, const uint8_t* ipa_r32, const uint8_t* ipa_z_head32, uint8_t* states208, uint8_t* out_proofs,
                               uint32_t* out_clocks) {
  const SamePermHead head{am48, vec_a32, perm, vec_a_blinders32, vec_m_blinders32};
  return gprod_chain(ctx, t, "cg1_same_perm_prove_device", same_perm_status_error, ell, n_blinders, n_provers, g_index, u_index, &head, nullptr, nullptr, nullptr,
                     vec_c_blinders32, ipa_r32, ipa_z_head32, states208, out_proofs, out_clocks);
}
}  // extern "C"
