// C ABI, part 11: the same-MSM argument proved on the device (kernels_same_msm.h over a cg1_fixed table for crs_G_vec and a light table,
// built inside the call, for the provers' vec_T | vec_U).  The body is cut into check | stage | absorb | args | reserve | enqueue parts,
// which the whole-shuffle entry (capi_shuffle.h) runs inside its own pipeline.
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

namespace {
struct SmsmLayout : ChainLayout {
  size_t gi, vx, vr, tu96, offs_a1, offs_a2, offs_l2, offs_l4;        // uploaded (the states: as they stand after the host's two lists)
  size_t x, k, row, chal, pts_a, pts_tu, tba, sca, tbl, scl;          // device only
};
SmsmLayout smsm_layout(size_t n, size_t P, size_t proof_bytes, size_t base = 0, size_t states_at = ChainLayout::OWN_STATES) {
  SmsmLayout L{};
  L.begin(base);
  L.gi = L.take(P * n * 4); L.vx = L.take(P * n * 32); L.vr = L.take(P * n * 32); L.tu96 = L.take(P * 2 * n * 96);
  L.offs_a1 = L.take((P + 1) * 4); L.offs_a2 = L.take((2 * P + 1) * 4); L.offs_l2 = L.take((2 * P + 1) * 4); L.offs_l4 = L.take((4 * P + 1) * 4);
  L.shared(P, proof_bytes, states_at);
  L.x = L.take(P * n * 32); L.k = L.take(P * n * 32); L.row = L.take(P * cg1smsm::SMSM_ROW); L.chal = L.take(P * 32);
  L.pts_a = L.take(P * 2 * 48); L.pts_tu = L.take(P * 4 * 48);
  L.tba = L.take(P * n * 4); L.sca = L.take(P * n * 32); L.tbl = L.take(P * 2 * n * 4); L.scl = L.take(P * 2 * n * 32);
  return L;
}

// ---- refusals: the whole call, before anything is written.  azz48 and vec_x32 null: absent (the whole-shuffle entry forms A', Z_t,
// Z_u and vec_x on the device).  head (with azz48): A, Z_t, Z_u as the transcript absorbs them; tu48: the 2 n encodings per prover
int smsm_check(cg1_ctx* ctx, const char* who, const cg1_fixed* t, bool pointers_ok, size_t n, size_t P, const uint32_t* g_index, const uint8_t* azz48,
               const uint8_t* tu_affine96, const uint8_t* vec_x32, const uint8_t* vec_r32, uint8_t* head, std::vector<uint8_t>& tu48) {
  static const char* const hashed[] = {"A", "Z_t", "Z_u"};
  if (const int rc = chain_check_shape(ctx, who, t, pointers_ok, n, CG1_SAME_MSM_MAX_N)) return rc;
  if (P > CG1_SAME_MSM_MAX_PROVERS || P * 2 * n > CG1_LIGHT_MAX_BASES) {
    snprintf(ctx->err, sizeof ctx->err, "%s: more than %d provers, or more than %d bases T | U, in one call", who, CG1_SAME_MSM_MAX_PROVERS, CG1_LIGHT_MAX_BASES);
    return CG1_ERR_ARG; }
  if (const int rc = chain_check_indices(ctx, who, t, {{g_index, P * n}})) return rc;
  if (const int rc = chain_check_scalars(ctx, who, {{vec_x32, P * n}, {vec_r32, P * n}})) return rc;
  std::vector<uint8_t> blobs(P * 2 * n * CG1_POINT_BYTES);
  tu48.resize(P * 2 * n * 48);
  if (azz48) { if (const int rc = chain_check_points(ctx, who, azz48, P, 3, hashed, head)) return rc; }       // A, Z_t, Z_u: only hashed, as re-serialised
  for (size_t b = 0; b < P * 2 * n; ++b) {                  // canonical coordinates, on the curve (or the all-zero identity record)
    const int rc = cg1_from_affine96(&blobs[b * CG1_POINT_BYTES], tu_affine96 + 96 * b, 1);
    if (rc != CG1_OK) { snprintf(ctx->err, sizeof ctx->err, "%s: prover %zu: entry %zu of vec_T | vec_U is not a curve point (status %d)", who, b / (2 * n), b % (2 * n), rc); return rc; }
  }
  cg1_batch_compress(tu48.data(), blobs.data(), P * 2 * n);
  return CG1_OK;
}
// ---- the inputs into the block (vec_x32 null: k_shuffle_begin writes the field on the device; vec_r32 null: a resident witness, placed
// on the device by k_whisk_witness_place)
void smsm_stage(uint8_t* H, const SmsmLayout& L, size_t n, size_t P, const uint32_t* g_index, const uint8_t* tu_affine96, const uint8_t* vec_x32, const uint8_t* vec_r32) {
  memcpy(H + L.gi, g_index, P * n * 4);
  if (vec_x32) memcpy(H + L.vx, vec_x32, P * n * 32);
  if (vec_r32) memcpy(H + L.vr, vec_r32, P * n * 32);
  memcpy(H + L.tu96, tu_affine96, P * 2 * n * 96);
  const uint32_t nn = (uint32_t)n, Pn = (uint32_t)P, hh = nn / 2;
  uint32_t* oa1 = reinterpret_cast<uint32_t*>(H + L.offs_a1);
  uint32_t* oa2 = reinterpret_cast<uint32_t*>(H + L.offs_a2);
  uint32_t* ol2 = reinterpret_cast<uint32_t*>(H + L.offs_l2);
  uint32_t* ol4 = reinterpret_cast<uint32_t*>(H + L.offs_l4);
  for (uint32_t i = 0; i <= Pn; ++i) oa1[i] = i * nn;
  for (uint32_t i = 0; i <= 2 * Pn; ++i) { oa2[i] = i * hh; ol2[i] = i * nn; }
  for (uint32_t i = 0; i <= 4 * Pn; ++i) ol4[i] = i * hh;
}
// The first two same_msm_step1 lists of one prover ([A, Z_t, Z_u] and vec_T + vec_U, 2 n encodings: ~74 Keccak permutations at n = 128)
// depend on nothing the chain computes: absorbed on the host, into the state that goes up.
void smsm_absorb(uint8_t* state208, const uint8_t* head144, const uint8_t* tu48, size_t n) {
  static const uint8_t step1[] = "same_msm_step1";
  cg1_merlin_append_list(state208, step1, 14, head144, 48, 3);
  cg1_merlin_append_list(state208, step1, 14, tu48, 48, 2 * n);
}
cg1smsm::SmsmArgs smsm_args(uint8_t* D, const SmsmLayout& L, size_t n, size_t pb, const cg1_fixed* t, const cg1_light* lt) {
  cg1smsm::SmsmArgs a;
  a.n0 = (uint32_t)n; a.lg = (uint32_t)chain_lg(n);
  a.gi = (const uint32_t*)(D + L.gi); a.vx = (const uint64_t*)(D + L.vx); a.vr = (const uint64_t*)(D + L.vr);
  a.x = (cg1fr::fr*)(D + L.x); a.k = (cg1fr::fr*)(D + L.k);
  a.states = D + L.states; a.row = D + L.row; a.chal = D + L.chal;
  a.pts_a = (const uint32_t*)(D + L.pts_a); a.pts_tu = (const uint32_t*)(D + L.pts_tu);
  a.proof = (uint32_t*)(D + L.proof); a.proof_words = (uint32_t)(pb / 4);
  a.tba = (uint32_t*)(D + L.tba); a.sca = (uint64_t*)(D + L.sca); a.tbl = (uint32_t*)(D + L.tbl); a.scl = (uint64_t*)(D + L.scl);
  a.status_a = t->d_status; a.status_tu = lt->d_status; a.chain_status = (uint32_t*)(D + L.status); a.clocks = (uint32_t*)(D + L.clocks);
  return a;
}
void smsm_shapes(const cg1_ctx* ctx, uint32_t Pn, uint32_t per_a, uint32_t mt, TableShape& sa, TableShape& sl) {
  sa = table_pick_shape<FixedKind>(ctx, per_a * Pn, mt);
  sl = table_pick_shape<LightKind>(ctx, 2 * per_a * Pn, mt);
}
// ---- the slice sums of the chain's largest launches (step B: n terms per MSM), reserved BEFORE the first launch: table_enqueue
// would otherwise free and allocate in mid-chain, which waits for the device
int smsm_reserve(cg1_ctx* ctx, cg1_fixed* t, cg1_light* lt, size_t n, size_t P) {
  const uint32_t nn = (uint32_t)n, Pn = (uint32_t)P, hh = nn / 2;
  size_t need_a = 0, need_l = 0;
  for (uint32_t per_a = 1; per_a <= 2; ++per_a) {
    const uint32_t mt = per_a == 1 ? nn : hh;
    TableShape sa, sl;
    smsm_shapes(ctx, Pn, per_a, mt, sa, sl);
    const size_t Sa = (mt + sa.slice - 1) / sa.slice, Sl = (mt + sl.slice - 1) / sl.slice;
    if (Sa > 1) need_a = std::max(need_a, (size_t)per_a * Pn * Sa);
    if (Sl > 1) need_l = std::max(need_l, (size_t)2 * per_a * Pn * Sl);
  }
  { const int rc = cg1::grow_device(ctx, t->d_partial, t->cap_partial, need_a, need_a); if (rc) return rc; }
  return cg1::grow_device(ctx, lt->d_partial, lt->cap_partial, need_l, need_l);
}
// ---- the chain: begin, build | MSMs finish stepB | (MSMs finish round) x lg n -- plain launches on the context's stream, no host wait
// between.  The first two launches read no transcript state; the rest starts from the states as smsm_absorb left them.
void smsm_enqueue_begin(cg1_ctx* ctx, cg1_light* lt, uint8_t* D, const SmsmLayout& L, const cg1smsm::SmsmArgs& a, size_t n, size_t P) {
  hipLaunchKernelGGL(cg1smsm::k_smsm_step, dim3((uint32_t)P), dim3(cg1smsm::SMSM_THREADS), 0, ctx->stream, a, cg1smsm::SMSM_BEGIN, (uint32_t)n, 0u);
  light_build(ctx, D + L.tu96, P * 2 * n, lt->d_tab);
}
int smsm_enqueue_rounds(cg1_ctx* ctx, cg1_fixed* t, cg1_light* lt, uint8_t* D, const SmsmLayout& L, const cg1smsm::SmsmArgs& a, size_t n, size_t P) {
  const uint32_t nn = (uint32_t)n, Pn = (uint32_t)P, hh = nn / 2;
  auto msms = [&](uint32_t per_a, uint32_t mt, const uint32_t* d_oa, const uint32_t* d_ol) -> int {
    const uint32_t Ma = per_a * Pn, Ml = 2 * per_a * Pn;
    TableShape sa, sl;
    smsm_shapes(ctx, Pn, per_a, mt, sa, sl);
    { const int rc = table_enqueue<FixedKind>(ctx, t, a.tba, (const uint32_t*)a.sca, d_oa, Ma, Pn * nn, mt, sa, false, nullptr, D + L.pts_a); if (rc) return rc; }
    return table_enqueue<LightKind>(ctx, lt, a.tbl, (const uint32_t*)a.scl, d_ol, Ml, Pn * 2 * nn, mt, sl, false, nullptr, D + L.pts_tu);
  };
  { const int rc = msms(1, nn, (const uint32_t*)(D + L.offs_a1), (const uint32_t*)(D + L.offs_l2)); if (rc) return rc; }
  hipLaunchKernelGGL(cg1smsm::k_smsm_step, dim3(Pn), dim3(cg1smsm::SMSM_THREADS), 0, ctx->stream, a, cg1smsm::SMSM_STEPB, nn, 0u);
  for (uint32_t r = 0; r < a.lg; ++r) {
    { const int rc = msms(2, hh, (const uint32_t*)(D + L.offs_a2), (const uint32_t*)(D + L.offs_l4)); if (rc) return rc; }
    hipLaunchKernelGGL(cg1smsm::k_smsm_step, dim3(Pn), dim3(cg1smsm::SMSM_THREADS), 0, ctx->stream, a, cg1smsm::SMSM_ROUND, nn >> r, r);
  }
  return CG1_OK;
}
}  // namespace

extern "C" {
size_t cg1_same_msm_proof_bytes(size_t n) { return chain_pow2(n) ? (3 + 6 * chain_lg(n)) * 48 + 32 : 0; }

int cg1_same_msm_prove_device(cg1_ctx* ctx, cg1_fixed* t, size_t n, size_t n_provers, const uint32_t* g_index, const uint8_t* azz48,
                              const uint8_t* tu_affine96, const uint8_t* vec_x32, const uint8_t* vec_r32, uint8_t* states208, uint8_t* out_proofs,
                              uint32_t* out_clocks) {
  static const char* const who = "cg1_same_msm_prove_device";
  if (!ctx) return CG1_ERR_HIP;
  if (n_provers == 0) return CG1_OK;
  const size_t P = n_provers;
  std::vector<uint8_t> head(P * 144), tu48;
  if (const int rc = smsm_check(ctx, who, t, g_index && azz48 && tu_affine96 && vec_x32 && vec_r32 && states208 && out_proofs, n, P, g_index, azz48, tu_affine96,
                                vec_x32, vec_r32, head.data(), tu48)) return rc;
  const size_t pb = cg1_same_msm_proof_bytes(n);
  const SmsmLayout L = smsm_layout(n, P, pb);
  uint8_t* H; uint8_t* D;
  if (const int rc = chain_stage(ctx, t, L, P, states208, H, D)) return rc;
  cg1_light* lt;
  if (const int rc = chain_light_scratch(ctx, t, P * 2 * n, lt)) return rc;
  // ---- stage the inputs: one block, one copy
  smsm_stage(H, L, n, P, g_index, tu_affine96, vec_x32, vec_r32);
  for (size_t p = 0; p < P; ++p) smsm_absorb(H + L.states + 208 * p, &head[144 * p], &tu48[p * 2 * n * 48], n);
  if (const int rc = chain_upload(ctx, t, L)) return rc;
  const cg1smsm::SmsmArgs a = smsm_args(D, L, n, pb, t, lt);
  if (const int rc = smsm_reserve(ctx, t, lt, n, P)) return rc;
  smsm_enqueue_begin(ctx, lt, D, L, a, n, P);
  if (const int rc = smsm_enqueue_rounds(ctx, t, lt, D, L, a, n, P)) return rc;
  return chain_finish(ctx, t, L, P, pb, states208, out_proofs, out_clocks);
}
}  // extern "C"
