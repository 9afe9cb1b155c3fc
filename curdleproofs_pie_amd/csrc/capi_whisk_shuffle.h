// C ABI, part 16: GenerateWhiskShuffleProof (whisk_interface.py:111-140) from tracker BYTES, for n_provers shuffles of one ell in step.
//   cg1_whisk_shuffle_front          the device front: decode and certify the 2 ell tracker points per prover, vec_T | vec_U = perm(k vec_R |
//                                    k vec_S) by k_whisk_permute_mul (kernels_whisk_shuffle.h), M as one k_table_msm over the CRS table --
//                                    one stream, one wait
//   cg1_whisk_shuffle_prove_device   the front, then cg1_shuffle_prove_device (capi_shuffle.h) on what it left, bases certified
// The refusals and their texts are shared with the host twin cg1_whisk_shuffle_front_emulate (whisk_shuffle_host.h, lazy_host.cpp).
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once
#include "whisk_shuffle_host.h"

namespace {
struct WhiskLayout : ChainLayout {
  size_t enc, perm, k, tb, sc, offs;                        // uploaded
  size_t wst;                                               // uploaded as zeros, read back: k_whisk_status's word
  size_t rs, tu, post, m48, st_dec, in_g1, st_msm;          // read back
};
WhiskLayout whisk_layout(size_t ell, size_t P) {
  WhiskLayout L{};
  L.begin(0);
  const size_t n = ell + cg1whisk_host::N_BLINDERS, pts = P * 2 * ell;
  L.enc = L.take(pts * 48); L.perm = L.take(P * ell * 4); L.k = L.take(P * 32);
  L.tb = L.take(P * n * 4); L.sc = L.take(P * n * 32); L.offs = L.take((P + 1) * 4);
  L.down_begin = L.total;
  L.wst = L.take(16);
  L.up_end = L.total;
  L.rs = L.take(pts * 96); L.tu = L.take(pts * 96); L.post = L.take(pts * 48); L.m48 = L.take(P * 48);
  L.st_dec = L.take(pts); L.in_g1 = L.take(pts); L.st_msm = L.take(16);
  L.down_end = L.total;
  return L;
}

// The front on the context's stream.  The outputs are host buffers of the caller's or of the whole call's; nothing is written into them
// before every refusal has been ruled out.
int whisk_front(cg1_ctx* ctx, const char* who, cg1_fixed* t, size_t ell, size_t P, const uint32_t* g_index, const uint32_t* h_index, const uint8_t* trackers96,
                const uint32_t* perm, const uint8_t* k32, const uint8_t* vec_m_blinders32, uint8_t* out_rs_affine96, uint8_t* out_tu_affine96, uint8_t* out_post96,
                uint8_t* out_m48) {
  constexpr size_t NB = cg1whisk_host::N_BLINDERS;
  if (const int rc = cg1whisk_host::check_shape(ctx->err, sizeof ctx->err, who, ell)) return rc;
  const size_t n = ell + NB, pts = P * 2 * ell;
  if (P > CG1_SAME_MSM_MAX_PROVERS || P * 2 * n > CG1_LIGHT_MAX_BASES) {
    snprintf(ctx->err, sizeof ctx->err, "%s: more than %d provers, or more than %d bases T | U, in one call", who, CG1_SAME_MSM_MAX_PROVERS, CG1_LIGHT_MAX_BASES);
    return CG1_ERR_ARG; }
  if (const int rc = chain_check_indices(ctx, who, t, {{g_index, P * ell}, {h_index, P * NB}})) return rc;
  if (const int rc = cg1whisk_host::check_inputs(ctx->err, sizeof ctx->err, who, ell, P, perm, k32, vec_m_blinders32)) return rc;

  // ---- the block
  const WhiskLayout L = whisk_layout(ell, P);
  uint8_t* H; uint8_t* D;
  if (const int rc = chain_reserve(ctx, t, L.total, H, D)) return rc;
  const uint32_t Pn = (uint32_t)P, nn = (uint32_t)n, np = (uint32_t)pts;
  const TableShape shape = table_pick_shape<FixedKind>(ctx, Pn, nn);
  {
    const size_t S = (nn + shape.slice - 1) / shape.slice, need = S > 1 ? (size_t)Pn * S : 0;
    if (const int rc = cg1::grow_device(ctx, t->d_partial, t->cap_partial, need, need)) return rc;
  }
  uint32_t* tb = reinterpret_cast<uint32_t*>(H + L.tb);
  uint32_t* offs = reinterpret_cast<uint32_t*>(H + L.offs);
  for (size_t p = 0; p < P; ++p) {
    uint8_t* enc = H + L.enc + p * 2 * ell * 48;            // r_G | k_r_G records -> vec_R | vec_S
    for (size_t i = 0; i < ell; ++i) {
      memcpy(enc + 48 * i, trackers96 + 96 * (p * ell + i), 48);
      memcpy(enc + 48 * (ell + i), trackers96 + 96 * (p * ell + i) + 48, 48);
    }
    memcpy(tb + p * n, g_index + p * ell, ell * 4); memcpy(tb + p * n + ell, h_index + p * NB, NB * 4);
    cg1whisk_host::m_scalar_row(ell, perm + p * ell, vec_m_blinders32 + 32 * NB * p, H + L.sc + 32 * n * p);
    offs[p] = (uint32_t)(p * n);
  }
  offs[P] = (uint32_t)(P * n);
  memcpy(H + L.perm, perm, P * ell * 4); memcpy(H + L.k, k32, P * 32);
  memset(H + L.wst, 0, 16);
  if (const int rc = chain_upload(ctx, t, L)) return rc;

  // ---- M for every prover as one launch over the CRS table; it depends on no tracker and runs ahead of the scalar multiplications
  if (const int rc = table_enqueue<FixedKind>(ctx, t, (const uint32_t*)(D + L.tb), (const uint32_t*)(D + L.sc), (const uint32_t*)(D + L.offs), Pn, Pn * nn, nn, shape, false,
                                              nullptr, D + L.m48)) return shuffle_refuse(ctx, rc);
  HIPCHK(hipMemcpyAsync(D + L.st_msm, t->d_status, 16, hipMemcpyDeviceToDevice, ctx->stream));
  // ---- decode, certify, the call's status word, then the multiplications
  hipLaunchKernelGGL(cg1::k_batch_decompress_row, dim3((np + 3u) / 4u), dim3(64), 0, ctx->stream, (const uint8_t*)(D + L.enc), (uint32_t*)(D + L.rs), D + L.st_dec, np);
  hipLaunchKernelGGL(cg1::k_subgroup_row, dim3(np), dim3(64), 0, ctx->stream, (const uint32_t*)(D + L.rs), np, D + L.in_g1);
  hipLaunchKernelGGL(cg1whisk::k_whisk_status, dim3(std::min<uint32_t>((np + 255u) / 256u, 64u)), dim3(256), 0, ctx->stream, (const uint8_t*)(D + L.st_dec),
                     (const uint8_t*)(D + L.in_g1), np, (uint32_t*)(D + L.wst));
  {
    cg1whisk::PermuteMulArgs a;
    a.ell = (uint32_t)ell; a.n_out = np;
    a.rs96 = (const uint32_t*)(D + L.rs); a.perm = (const uint32_t*)(D + L.perm); a.k = (const uint32_t*)(D + L.k); a.status = (const uint32_t*)(D + L.wst);
    a.tu96 = (uint32_t*)(D + L.tu); a.post48 = (uint32_t*)(D + L.post);
    hipLaunchKernelGGL(cg1whisk::k_whisk_permute_mul, dim3(np), dim3(64), 0, ctx->stream, a);
  }
  // ---- one copy down, the one wait, the status words, and only then the caller's buffers
  if (const int rc = chain_download(ctx, t, L)) return shuffle_refuse(ctx, rc);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  for (int pass = 0; pass < 2; ++pass)                      // the decoder's refusals first, then the subgroup test's, each in tracker order
    for (size_t p = 0; p < P; ++p)
      for (size_t i = 0; i < ell; ++i)
        for (int half = 0; half < 2; ++half) {
          const size_t at = p * 2 * ell + half * ell + i;
          if (pass == 0 && H[L.st_dec + at]) return cg1whisk_host::refuse_point(ctx->err, sizeof ctx->err, who, p, i, half, H[L.st_dec + at]);
          if (pass == 1 && !H[L.in_g1 + at]) return cg1whisk_host::refuse_point(ctx->err, sizeof ctx->err, who, p, i, half, CG1_ERR_NOT_IN_SUBGROUP);
        }
  if (reinterpret_cast<const uint32_t*>(H + L.wst)[0]) { snprintf(ctx->err, sizeof ctx->err, "%s: the device refused the call's points, but no point's status says why", who); return CG1_ERR_HIP; }
  if (const int rc = table_status_error<FixedKind>(ctx, reinterpret_cast<const uint32_t*>(H + L.st_msm)[0])) return rc;
  memcpy(out_rs_affine96, H + L.rs, pts * 96); memcpy(out_tu_affine96, H + L.tu, pts * 96);
  memcpy(out_post96, H + L.post, pts * 48); memcpy(out_m48, H + L.m48, P * 48);
  return CG1_OK;
}
}  // namespace

extern "C" {
size_t cg1_whisk_shuffle_proof_bytes(size_t ell) {
  const size_t pb = cg1_shuffle_prover_proof_bytes(ell);
  return pb ? 48 + pb : 0;
}

int cg1_whisk_shuffle_front(cg1_ctx* ctx, cg1_fixed* t, size_t ell, size_t n_provers, const uint32_t* g_index, const uint32_t* h_index, const uint8_t* trackers96,
                            const uint32_t* perm, const uint8_t* k32, const uint8_t* vec_m_blinders32, uint8_t* out_rs_affine96, uint8_t* out_tu_affine96,
                            uint8_t* out_post96, uint8_t* out_m48) {
  static const char* const who = "cg1_whisk_shuffle_front";
  if (!ctx) return CG1_ERR_HIP;
  if (n_provers == 0) return CG1_OK;
  const bool pointers_ok = g_index && h_index && trackers96 && perm && k32 && vec_m_blinders32 && out_rs_affine96 && out_tu_affine96 && out_post96 && out_m48;
  if (!t || t->device != ctx->device || !pointers_ok) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", who); return CG1_ERR_ARG; }
  return whisk_front(ctx, who, t, ell, n_provers, g_index, h_index, trackers96, perm, k32, vec_m_blinders32, out_rs_affine96, out_tu_affine96, out_post96, out_m48);
}

int cg1_whisk_shuffle_prove_device(cg1_ctx* ctx, cg1_fixed* t, size_t ell, size_t n_provers, const uint32_t* g_index, const uint32_t* h_index, const uint32_t* u_index,
                                   const uint32_t* gt_index, const uint32_t* gu_index, const uint8_t* gth_affine96, const uint8_t* trackers96, const uint32_t* perm,
                                   const uint8_t* k32, const uint8_t* vec_m_blinders32, const uint8_t* vec_a_blinders32, const uint8_t* vec_c_blinders32,
                                   const uint8_t* ipa_r32, const uint8_t* ipa_z_head32, const uint8_t* blinders32, const uint8_t* vec_r32, uint8_t* out_post96,
                                   uint8_t* out_proofs) {
  static const char* const who = "cg1_whisk_shuffle_prove_device";
  static const char* const chain = "cg1_shuffle_prove_device";
  if (!ctx) return CG1_ERR_HIP;
  if (n_provers == 0) return CG1_OK;
  const bool pointers_ok = g_index && h_index && u_index && gt_index && gu_index && gth_affine96 && trackers96 && perm && k32 && vec_m_blinders32 && vec_a_blinders32 &&
                           vec_c_blinders32 && ipa_r32 && ipa_z_head32 && blinders32 && vec_r32 && out_post96 && out_proofs;
  if (!t || t->device != ctx->device || !pointers_ok) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", who); return CG1_ERR_ARG; }
  // both halves write into scratch of this call's; the caller's buffers are touched only when neither has refused.  (A shape or a P
  // the front refuses gets no scratch: the front refuses them before it writes.)
  const size_t P = n_provers, pts = cg1whisk_host::shape_ok(ell) && P <= CG1_SAME_MSM_MAX_PROVERS ? P * 2 * ell : 0;
  std::vector<uint8_t> rs(pts * 96), tu(pts * 96), post(pts * 48), m48(pts ? P * 48 : 0), proofs;
  if (const int rc = whisk_front(ctx, who, t, ell, P, g_index, h_index, trackers96, perm, k32, vec_m_blinders32, rs.data(), tu.data(), post.data(), m48.data())) return rc;
  const size_t pb = cg1_shuffle_prover_proof_bytes(ell);
  proofs.resize(P * pb);
  if (const int rc = cg1_shuffle_prove_device(ctx, t, ell, P, g_index, h_index, u_index, gt_index, gu_index, gth_affine96, rs.data(), tu.data(), m48.data(), perm, k32,
                                              vec_m_blinders32, vec_a_blinders32, vec_c_blinders32, ipa_r32, ipa_z_head32, blinders32, vec_r32, 1, proofs.data(), nullptr)) {
    const size_t cl = strlen(chain);                        // the chain's text under this entry's name
    if (strncmp(ctx->err, chain, cl) == 0) {
      const std::string tail(ctx->err + cl);
      snprintf(ctx->err, sizeof ctx->err, "%s%s", who, tail.c_str());
    }
    return rc;
  }
  memcpy(out_post96, post.data(), pts * 48);
  for (size_t p = 0; p < P; ++p) {                          // M || proof: the wire form cg1_shuffle_proof_bytes counts
    memcpy(out_proofs + p * (48 + pb), &m48[48 * p], 48);
    memcpy(out_proofs + p * (48 + pb) + 48, &proofs[p * pb], pb);
  }
  return CG1_OK;
}
}  // extern "C"
