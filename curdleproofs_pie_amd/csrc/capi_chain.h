// The host layer every argument proved as one device launch chain shares (capi_ipa.h, capi_same_msm.h, capi_gprod.h with capi_same_perm.h, capi_same_scalar.h): the layout of the staging block,
// the refusals, the staging of status, clocks and states, and the tail from the download to the caller's buffers.  An entry point keeps
// its argument list, its layout's fields, its own refusals and its launch sequence.
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

namespace {
// Byte offsets into a table handle's ONE staging block (t->h_chain, pinned, and its device twin t->d_chain: the same layout).  The calls
// on a handle run under the context's lock and complete before they return, and each lays the block out afresh: nothing in it survives
// from one call to the next.  Sections, in order: uploaded | uploaded and read back | read back (both: shared()) | device only.
// A call that runs several arguments (capi_shuffle.h) lays their layouts end to end -- begin(base) -- with ONE states field in front of them
// (shared(.., states_at)): every argument then uploads [up_begin, up_end) and downloads [down_begin, down_end) of its own.
struct ChainLayout {
  static constexpr size_t OWN_STATES = ~(size_t)0;
  size_t status = 0, clocks = 0, states = 0, proof = 0;     // zeros | zeros | the callers' states, up and down | the proofs, down
  size_t up_begin = 0, up_end = 0, down_begin = 0, down_end = 0, total = 0;
  void begin(size_t base) { up_begin = total = base; }
  size_t take(size_t bytes) { const size_t at = total; total = (total + bytes + 63) & ~(size_t)63; return at; }
  void shared(size_t P, size_t proof_bytes, size_t states_at = OWN_STATES) {      // between the uploaded and the device-only fields
    down_begin = total;
    status = take(16); clocks = take(P * 16); states = states_at == OWN_STATES ? take(P * 208) : states_at;
    up_end = total;
    proof = take(P * proof_bytes);
    down_end = total;
  }
};

size_t chain_lg(size_t n) {
  size_t lg = 0;
  while (((size_t)1 << lg) < n) ++lg;
  return lg;
}
bool chain_pow2(size_t n) { return n >= 2 && (n & (n - 1)) == 0; }

// ---- the refusals every entry makes, in the order the entries make them; `who` is the entry's name, so the texts are its own
int chain_check_shape(cg1_ctx* ctx, const char* who, const cg1_fixed* t, bool pointers_ok, size_t n, int max_n) {
  if (!t || t->device != ctx->device || !pointers_ok) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", who); return CG1_ERR_ARG; }
  if (!chain_pow2(n) || n > (size_t)max_n) { snprintf(ctx->err, sizeof ctx->err, "%s: n must be a power of two in 2 .. %d", who, max_n); return CG1_ERR_ARG; }
  return CG1_OK;
}
int chain_check_indices(cg1_ctx* ctx, const char* who, const cg1_fixed* t, std::initializer_list<std::pair<const uint32_t*, size_t>> lists) {
  for (const auto& l : lists)
    for (size_t i = 0; i < l.second; ++i)
      if (l.first[i] >= t->n_bases) { snprintf(ctx->err, sizeof ctx->err, "%s: a base index is outside the table", who); return CG1_ERR_ARG; }
  return CG1_OK;
}
int chain_check_scalars(cg1_ctx* ctx, const char* who, std::initializer_list<std::pair<const uint8_t*, size_t>> lists) {       // a null list is an absent one
  for (const auto& l : lists)
    for (size_t i = 0; l.first && i < l.second; ++i) {
      uint32_t w[8];
      memcpy(w, l.first + 32 * i, 32);
      if (!cg1::fixed_scalar_below_r(w)) { snprintf(ctx->err, sizeof ctx->err, "%s: a scalar is >= r: scalar32 must be a canonical Fr element", who); return CG1_ERR_ENCODING; }
    }
  return CG1_OK;
}
// the points a prover only hashes: `per` encodings each, named names[0 .. per).  canon (optional): a copy as the transcript absorbs them,
// the identity re-serialised (util.py:27-32)
int chain_check_points(cg1_ctx* ctx, const char* who, const uint8_t* pts48, size_t P, size_t per, const char* const* names, uint8_t* canon) {
  for (size_t i = 0; i < per * P; ++i) {
    int inf = 0;
    const int rc = cg1_validate_compressed(pts48 + 48 * i, &inf);
    if (rc != CG1_OK) { snprintf(ctx->err, sizeof ctx->err, "%s: prover %zu: %s does not decode (status %d)", who, i / per, names[i % per], rc); return rc; }
    if (canon) {
      memcpy(canon + 48 * i, pts48 + 48 * i, 48);
      if (inf) { memset(canon + 48 * i, 0, 48); canon[48 * i] = 0xC0; }
    }
  }
  return CG1_OK;
}

// ---- after the refusals: the block, laid out by L, with its shared upload fields filled (status and clocks zero, the states as given)
int chain_reserve(cg1_ctx* ctx, cg1_fixed* t, size_t total, uint8_t*& H, uint8_t*& D) {
  HIPCHK(hipSetDevice(ctx->device));
  ctx->pend.active = false;
  { const int rc = cg1::grow_pinned_pair(ctx, t->h_chain, nullptr, t->d_chain, t->cap_chain, total, total, hipHostMallocDefault); if (rc) return rc; }
  H = t->h_chain; D = t->d_chain;
  t->chain_used = std::max(t->chain_used, total);
  return CG1_OK;
}
void chain_clear(uint8_t* H, const ChainLayout& L, size_t P) { memset(H + L.status, 0, 16); memset(H + L.clocks, 0, P * 16); }
int chain_stage(cg1_ctx* ctx, cg1_fixed* t, const ChainLayout& L, size_t P, const uint8_t* states208, uint8_t*& H, uint8_t*& D) {
  if (const int rc = chain_reserve(ctx, t, L.total, H, D)) return rc;
  chain_clear(H, L, P);
  memcpy(H + L.states, states208, P * 208);
  return CG1_OK;
}
// the two copies of a layout, enqueued on the context's stream; nothing waits here
int chain_upload(cg1_ctx* ctx, cg1_fixed* t, const ChainLayout& L) {
  HIPCHK(hipMemcpyAsync(t->d_chain + L.up_begin, t->h_chain + L.up_begin, L.up_end - L.up_begin, hipMemcpyHostToDevice, ctx->stream));
  return CG1_OK;
}
int chain_download(cg1_ctx* ctx, cg1_fixed* t, const ChainLayout& L) {
  HIPCHK(hipMemcpyAsync(t->h_chain + L.down_begin, t->d_chain + L.down_begin, L.down_end - L.down_begin, hipMemcpyDeviceToHost, ctx->stream));
  return CG1_OK;
}
// the refusals of a chain whose status word has come down.  own_status (optional): those of an argument whose step kernel sets status
// bits of its own, above k_table_msm's; `who` is the entry's name in their texts
using ChainOwnStatus = int (*)(cg1_ctx*, const char* who, uint32_t);
int chain_status_error(cg1_ctx* ctx, const uint8_t* H, const ChainLayout& L, const char* who, ChainOwnStatus own_status) {
  const uint32_t st = reinterpret_cast<const uint32_t*>(H + L.status)[0];
  { const int rc = table_status_error<FixedKind>(ctx, st); if (rc) return rc; }
  return own_status ? own_status(ctx, who, st) : CG1_OK;
}
// ---- after the last launch: one copy down, the one wait, the chain's status, and only then the caller's buffers
int chain_finish(cg1_ctx* ctx, cg1_fixed* t, const ChainLayout& L, size_t P, size_t proof_bytes, uint8_t* states208, uint8_t* out_proofs, uint32_t* out_clocks,
                 const char* who = nullptr, ChainOwnStatus own_status = nullptr) {
  uint8_t* H = t->h_chain;
  if (const int rc = chain_download(ctx, t, L)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));                 // the one wait
  HIPCHK(hipGetLastError());
  if (const int rc = chain_status_error(ctx, H, L, who, own_status)) return rc;
  memcpy(out_proofs, H + L.proof, P * proof_bytes);
  memcpy(states208, H + L.states, P * 208);
  if (out_clocks) memcpy(out_clocks, H + L.clocks, P * 16);
  return CG1_OK;
}
}  // namespace
