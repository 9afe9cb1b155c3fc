// C ABI, part 16: GenerateWhiskShuffleProof (whisk_interface.py:111-140) from tracker BYTES, for n_provers shuffles of one ell in step.
//   cg1_whisk_shuffle_front          the device front: decode and certify the 2 ell tracker points per prover, vec_T | vec_U = perm(k vec_R |
//                                    k vec_S) by k_whisk_permute_mul (kernels_whisk_shuffle.h), M as one k_table_msm over the CRS table --
//                                    one stream, one wait
//   cg1_whisk_shuffle_prove_device   the front, then shuffle_prove (capi_shuffle.h) on what it left, bases certified
//   cg1_whisk_shuffle_draws_device   permutation, k and every blinder of n_provers shuffles from a 32-byte seed (k_whisk_draws, k_whisk_fisher_yates)
//   cg1_whisk_shuffle_prove_seeded   those draws, the front with a status PER PROVER, and the chain on the provers the front did not refuse
// The refusals and their texts are shared with the host twin cg1_whisk_shuffle_front_emulate (whisk_shuffle_host.h, lazy_host.cpp).
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once
#include "whisk_shuffle_host.h"

namespace {
struct WhiskLayout : ChainLayout {
  size_t enc, perm, k, tb, sc, offs;                        // uploaded
  size_t wst;                                               // uploaded as zeros, read back: k_whisk_status's word
  size_t rs, tu, post, m48, st_dec, in_g1, st_msm, pst;     // read back (pst: k_whisk_status_provers' words)
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
  L.st_dec = L.take(pts); L.in_g1 = L.take(pts); L.st_msm = L.take(16); L.pst = L.take(P * 4);
  L.down_end = L.total;
  return L;
}

// M = sum perm[i] G_i + sum vec_m_blinders[b] H_b of every prover as ONE k_table_msm launch over the CRS table, for whisk_front and the chain
// prover (capi_chain_prove.h): the fields of the caller's layout it uses, the host rows, the launch.
struct WhiskMFields { size_t tb, sc, offs, m48, st_msm; };
TableShape whisk_m_shape(cg1_ctx* ctx, cg1_fixed* t, size_t ell, size_t P, int& rc) {
  const uint32_t Pn = (uint32_t)P, nn = (uint32_t)(ell + cg1whisk_host::N_BLINDERS);
  const TableShape shape = table_pick_shape<FixedKind>(ctx, Pn, nn);
  const size_t S = (nn + shape.slice - 1) / shape.slice, need = S > 1 ? (size_t)Pn * S : 0;
  rc = cg1::grow_device(ctx, t->d_partial, t->cap_partial, need, need);
  return shape;
}
void whisk_m_rows(uint8_t* H, const WhiskMFields& F, size_t ell, size_t P, const uint32_t* g_index, const uint32_t* h_index, const uint32_t* perm,
                  const uint8_t* vec_m_blinders32) {
  constexpr size_t NB = cg1whisk_host::N_BLINDERS;
  const size_t n = ell + NB;
  uint32_t* tb = reinterpret_cast<uint32_t*>(H + F.tb);
  uint32_t* offs = reinterpret_cast<uint32_t*>(H + F.offs);
  for (size_t p = 0; p < P; ++p) {
    memcpy(tb + p * n, g_index + p * ell, ell * 4); memcpy(tb + p * n + ell, h_index + p * NB, NB * 4);
    if (perm) cg1whisk_host::m_scalar_row(ell, perm + p * ell, vec_m_blinders32 + 32 * NB * p, H + F.sc + 32 * n * p);      // (null: a resident witness, placed on the device)
    offs[p] = (uint32_t)(p * n);
  }
  offs[P] = (uint32_t)(P * n);
}
int whisk_m_enqueue(cg1_ctx* ctx, cg1_fixed* t, uint8_t* D, const WhiskMFields& F, size_t ell, size_t P, const TableShape& shape) {
  const uint32_t Pn = (uint32_t)P, nn = (uint32_t)(ell + cg1whisk_host::N_BLINDERS);
  if (const int rc = table_enqueue<FixedKind>(ctx, t, (const uint32_t*)(D + F.tb), (const uint32_t*)(D + F.sc), (const uint32_t*)(D + F.offs), Pn, Pn * nn, nn, shape, false,
                                              nullptr, D + F.m48)) return shuffle_refuse(ctx, rc);
  HIPCHK(hipMemcpyAsync(D + F.st_msm, t->d_status, 16, hipMemcpyDeviceToDevice, ctx->stream));
  return CG1_OK;
}

// the witness fields of the front's block as the host stages them, and the public rows of M beside them -> the witness bytes written
// (a resident witness: none, its fields stay as they lie)
size_t whisk_front_stage(uint8_t* H, const WhiskLayout& L, const WhiskMFields& MF, size_t ell, size_t P, const uint32_t* g_index, const uint32_t* h_index,
                         const ShuffleWitness& w) {
  whisk_m_rows(H, MF, ell, P, g_index, h_index, w.perm, w.col[cg1whisk_host::COL_MBL]);
  if (w.resident()) return 0;
  memcpy(H + L.perm, w.perm, P * ell * 4); memcpy(H + L.k, w.col[cg1whisk_host::COL_K], P * 32);
  return cg1whisk_host::place_bytes(cg1whisk_host::BLOCK_FRONT, ell, P);
}
void whisk_front_place_at(size_t* at, const WhiskLayout& L) {
  at[cg1whisk_host::PF_L_PERM] = L.perm; at[cg1whisk_host::PF_L_K] = L.k; at[cg1whisk_host::PF_MF_SC] = L.sc;
}

// The front on the context's stream.  The outputs are host buffers of the caller's or of the whole call's; nothing is written into them
// before every refusal has been ruled out.  out_status / out_bad_at (both or neither): a tracker point that does not decode or lies
// outside G1 then refuses ITS prover only -- code and tracker 2 + half of its first such point; its four outputs are zeros -- and the call
// goes on for the others.  The witness: its permutations, COL_K and COL_MBL (a host view needs no other column).  A resident one is
// placed into the block on the device, behind the upload and in front of the first kernel; check_inputs is skipped for it, which is sound
// for the reasons shuffle_prove gives (capi_shuffle.h): the device's own draws are reduced mod r and are permutations by construction.
int whisk_front(cg1_ctx* ctx, const char* who, cg1_fixed* t, size_t ell, size_t P, const uint32_t* g_index, const uint32_t* h_index, const uint8_t* trackers96,
                const ShuffleWitness& witness, uint8_t* out_rs_affine96, uint8_t* out_tu_affine96, uint8_t* out_post96,
                uint8_t* out_m48, int32_t* out_status = nullptr, uint32_t* out_bad_at = nullptr) {
  constexpr size_t NB = cg1whisk_host::N_BLINDERS;
  if (const int rc = cg1whisk_host::check_shape(ctx->err, sizeof ctx->err, who, ell)) return rc;
  const size_t n = ell + NB, pts = P * 2 * ell;
  if (P > CG1_SAME_MSM_MAX_PROVERS || P * 2 * n > CG1_LIGHT_MAX_BASES) {
    snprintf(ctx->err, sizeof ctx->err, "%s: more than %d provers, or more than %d bases T | U, in one call", who, CG1_SAME_MSM_MAX_PROVERS, CG1_LIGHT_MAX_BASES);
    return CG1_ERR_ARG; }
  if (const int rc = chain_check_indices(ctx, who, t, {{g_index, P * ell}, {h_index, P * NB}})) return rc;
  if (!witness.resident()) {
    if (const int rc = cg1whisk_host::check_inputs(ctx->err, sizeof ctx->err, who, ell, P, witness.perm, witness.col[cg1whisk_host::COL_K], witness.col[cg1whisk_host::COL_MBL])) return rc;
  }

  // ---- the block
  const WhiskLayout L = whisk_layout(ell, P);
  uint8_t* H; uint8_t* D;
  if (const int rc = chain_reserve(ctx, t, L.total, H, D)) return rc;
  const uint32_t Pn = (uint32_t)P, np = (uint32_t)pts;
  int shape_rc = CG1_OK;
  const TableShape shape = whisk_m_shape(ctx, t, ell, P, shape_rc);
  if (shape_rc) return shape_rc;
  const WhiskMFields MF{L.tb, L.sc, L.offs, L.m48, L.st_msm};
  for (size_t p = 0; p < P; ++p) {
    uint8_t* enc = H + L.enc + p * 2 * ell * 48;            // r_G | k_r_G records -> vec_R | vec_S
    for (size_t i = 0; i < ell; ++i) {
      memcpy(enc + 48 * i, trackers96 + 96 * (p * ell + i), 48);
      memcpy(enc + 48 * (ell + i), trackers96 + 96 * (p * ell + i) + 48, 48);
    }
  }
  ctx->whisk_traffic[1] += whisk_front_stage(H, L, MF, ell, P, g_index, h_index, witness);
  memset(H + L.wst, 0, 16);
  if (const int rc = chain_upload(ctx, t, L)) return rc;
  if (witness.resident()) {
    size_t at[cg1whisk_host::N_PLACE_FIELDS] = {0};
    whisk_front_place_at(at, L);
    if (const int rc = whisk_place_enqueue(ctx, D, witness, cg1whisk_host::BLOCK_FRONT, 0, at)) return shuffle_refuse(ctx, rc);
  }

  // ---- M for every prover as one launch over the CRS table; it depends on no tracker and runs ahead of the scalar multiplications
  if (const int rc = whisk_m_enqueue(ctx, t, D, MF, ell, P, shape)) return rc;
  // ---- decode, certify, the call's status word, then the multiplications
  hipLaunchKernelGGL(cg1::k_batch_decompress_row, dim3((np + 3u) / 4u), dim3(64), 0, ctx->stream, (const uint8_t*)(D + L.enc), (uint32_t*)(D + L.rs), D + L.st_dec, np);
  hipLaunchKernelGGL(cg1::k_subgroup_row, dim3(np), dim3(64), 0, ctx->stream, (const uint32_t*)(D + L.rs), np, D + L.in_g1);
  if (out_status)
    hipLaunchKernelGGL(cg1whisk::k_whisk_status_provers, dim3(Pn), dim3(64), 0, ctx->stream, (const uint8_t*)(D + L.st_dec), (const uint8_t*)(D + L.in_g1), (uint32_t)ell,
                       (uint32_t*)(D + L.pst));
  else
    hipLaunchKernelGGL(cg1whisk::k_whisk_status, dim3(std::min<uint32_t>((np + 255u) / 256u, 64u)), dim3(256), 0, ctx->stream, (const uint8_t*)(D + L.st_dec),
                       (const uint8_t*)(D + L.in_g1), np, (uint32_t*)(D + L.wst));
  {
    cg1whisk::PermuteMulArgs a;
    a.ell = (uint32_t)ell; a.n_out = np;
    a.rs96 = (const uint32_t*)(D + L.rs); a.perm = (const uint32_t*)(D + L.perm); a.k = (const uint32_t*)(D + L.k); a.status = (const uint32_t*)(D + L.wst);
    a.prover_status = out_status ? (const uint32_t*)(D + L.pst) : nullptr;
    a.tu96 = (uint32_t*)(D + L.tu); a.post48 = (uint32_t*)(D + L.post);
    hipLaunchKernelGGL(cg1whisk::k_whisk_permute_mul, dim3(np), dim3(64), 0, ctx->stream, a);
  }
  // ---- one copy down, the one wait, the status words, and only then the caller's buffers
  if (const int rc = chain_download(ctx, t, L)) return shuffle_refuse(ctx, rc);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  for (int pass = 0; pass < 2 && !out_status; ++pass)       // the decoder's refusals first, then the subgroup test's, each in tracker order
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
  for (size_t p = 0; out_status && p < P; ++p) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(H + L.pst)[p];
    out_status[p] = (int32_t)(w >> 16); out_bad_at[p] = w & 0xffffu;
    if (!w) continue;                                       // (k_whisk_permute_mul wrote nothing for it: the block holds an earlier call's bytes there)
    memset(out_rs_affine96 + p * 2 * ell * 96, 0, 2 * ell * 96); memset(out_tu_affine96 + p * 2 * ell * 96, 0, 2 * ell * 96);
    memset(out_post96 + p * 2 * ell * 48, 0, 2 * ell * 48); memset(out_m48 + p * 48, 0, 48);
  }
  return CG1_OK;
}

// M alone, for the chain prover, whose trackers come from its own stage: the block laid out for M only, one launch, one copy down, one
// wait.  (whisk_front runs the same pieces fused with the decode, under its one wait.)
int whisk_m_run(cg1_ctx* ctx, const char* who, cg1_fixed* t, size_t ell, size_t Q, const ShuffleCrsRows& rows, const ShuffleWitness& witness, uint8_t* out_m48) {
  const size_t n = ell + cg1whisk_host::N_BLINDERS;
  struct MLayout : ChainLayout { WhiskMFields f; } ML{};
  ML.begin(0);
  ML.f.tb = ML.take(Q * n * 4); ML.f.sc = ML.take(Q * n * 32); ML.f.offs = ML.take((Q + 1) * 4);
  ML.up_end = ML.down_begin = ML.total;
  ML.f.m48 = ML.take(Q * 48); ML.f.st_msm = ML.take(16);
  ML.down_end = ML.total;
  uint8_t* H; uint8_t* D;
  if (const int rc = chain_reserve(ctx, t, ML.total, H, D)) return rc;
  int shape_rc = CG1_OK;
  const TableShape shape = whisk_m_shape(ctx, t, ell, Q, shape_rc);
  if (shape_rc) return shape_rc;
  whisk_m_rows(H, ML.f, ell, Q, rows.g, rows.h, witness.perm, witness.col[cg1whisk_host::COL_MBL]);
  if (const int rc = chain_upload(ctx, t, ML)) return rc;
  if (const int rc = whisk_m_enqueue(ctx, t, D, ML.f, ell, Q, shape)) return rc;
  if (const int rc = chain_download(ctx, t, ML)) return shuffle_refuse(ctx, rc);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess) { snprintf(ctx->err, sizeof ctx->err, "%s: the device failed under M", who); return CG1_ERR_HIP; }
  if (const int rc = table_status_error<FixedKind>(ctx, reinterpret_cast<const uint32_t*>(H + ML.f.st_msm)[0])) return rc;
  memcpy(out_m48, H + ML.f.m48, Q * 48);
  return CG1_OK;
}

// M || proof of prover p: the wire form cg1_whisk_shuffle_proof_bytes counts (pb = cg1_shuffle_prover_proof_bytes(ell))
void whisk_write_wire(uint8_t* out_proofs, size_t p, const uint8_t* m48, const uint8_t* proof, size_t pb) {
  memcpy(out_proofs + p * (48 + pb), m48, 48);
  memcpy(out_proofs + p * (48 + pb) + 48, proof, pb);
}
// The caller's two buffers: zeros for all P provers, then kept prover q at position keep[q] (keep == NULL: q) -- its post trackers
// (post96: P rows, by position), its M and its proof (m48, proofs: Q rows, as the chain took them).
void whisk_place_outputs(size_t ell, size_t P, const size_t* keep, size_t Q, const uint8_t* post96, const uint8_t* m48, const uint8_t* proofs, uint8_t* out_post96,
                         uint8_t* out_proofs) {
  const size_t pb = cg1_shuffle_prover_proof_bytes(ell), row = 2 * ell * 48;
  memset(out_post96, 0, P * row); memset(out_proofs, 0, P * (48 + pb));
  for (size_t q = 0; q < Q; ++q) {
    const size_t p = keep ? keep[q] : q;
    memcpy(out_post96 + p * row, post96 + p * row, row);
    whisk_write_wire(out_proofs, p, m48 + 48 * q, proofs + q * pb, pb);
  }
}

// ---- the seeded draws
using cg1whisk_host::DrawBlock;
// k_whisk_draws and k_whisk_fisher_yates on the context's stream, into ctx->d_whisk_draws (grown here), and nothing else: no copy, no
// zeroing, no wait.  The arguments have been checked (cg1whisk_host::check_draws).  This is the whole of the RESIDENT form of the draws:
// they stay in the buffer for k_whisk_witness_place to read, in stream order, and whoever calls this for them holds a WhiskDrawsWipe.
int whisk_draws_enqueue(cg1_ctx* ctx, size_t ell, size_t P, const uint8_t* seed32, uint64_t first_index) {
  const DrawBlock B = cg1whisk_host::draw_block(ell, P);
  HIPCHK(hipSetDevice(ctx->device));
  if (const int rc = cg1::grow_bufs(ctx, ctx->cap_whisk_draws, B.total, B.total, {cg1::dev_buf(ctx->d_whisk_draws, B.total)})) return rc;
  uint8_t* D = (uint8_t*)ctx->d_whisk_draws;
  cg1whisk::DrawArgs a;
  memcpy(a.seed.w, seed32, 32);
  a.ell = (uint32_t)ell; a.n_provers = (uint32_t)P; a.first_index = (uint32_t)first_index;      // (first_index = 2^32 only with P = 0)
  a.swaps = (uint32_t*)(D + B.swaps); a.scalars = (uint32_t*)(D + B.scalars);
  const uint32_t lanes = (uint32_t)P * cg1whisk_host::draw_count((uint32_t)ell);
  hipLaunchKernelGGL(cg1whisk::k_whisk_draws, dim3((lanes + cg1merlin::LANES - 1) / cg1merlin::LANES), dim3(cg1merlin::LANES), 0, ctx->stream, a);
  hipLaunchKernelGGL(cg1whisk::k_whisk_fisher_yates, dim3((uint32_t)P), dim3(64), 0, ctx->stream, (const uint32_t*)(D + B.swaps), (uint32_t)ell, (uint32_t*)(D + B.perm));
  cg1::wipe(&a, sizeof a);
  return CG1_OK;
}
// The copying form: those kernels, ONE copy down (perm | scalars -> stage), the device buffer zeroed, one wait.
int whisk_draws_run(cg1_ctx* ctx, size_t ell, size_t P, const uint8_t* seed32, uint64_t first_index, cg1::WipedBytes& stage) {
  const DrawBlock B = cg1whisk_host::draw_block(ell, P);
  if (const int rc = whisk_draws_enqueue(ctx, ell, P, seed32, first_index)) return rc;
  uint8_t* D = (uint8_t*)ctx->d_whisk_draws;
  stage.v.resize(B.total - B.perm);
  ctx->whisk_traffic[0] += B.total - B.perm; ctx->whisk_traffic[1] += B.total - B.perm;
  hipError_t e = hipMemcpyAsync(stage.v.data(), D + B.perm, B.total - B.perm, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e2 = hipMemsetAsync(D, 0, B.total, ctx->stream);        // the draws do not outlive the call on the device, whatever the copy said
  const hipError_t e3 = hipStreamSynchronize(ctx->stream);
  e = e != hipSuccess ? e : e2 != hipSuccess ? e2 : e3;
  HIPCHK(e);
  HIPCHK(hipGetLastError());
  return CG1_OK;
}
// The scope guard of a resident seeded call: the context's draws buffer, all of it, zeroed behind whatever the stream still holds, and
// waited for -- on success, on every refusal of whisk_front / shuffle_prove, on a HIP error and on a growth that failed (which leaves
// no buffer: nothing to zero).
struct WhiskDrawsWipe {
  cg1_ctx* ctx;
  explicit WhiskDrawsWipe(cg1_ctx* c) : ctx(c) {}          // (null: the copying path, whose whisk_draws_run has zeroed the buffer itself)
  WhiskDrawsWipe(const WhiskDrawsWipe&) = delete;
  ~WhiskDrawsWipe() {
    if (!ctx || !ctx->d_whisk_draws || !ctx->cap_whisk_draws) return;
    (void)hipMemsetAsync(ctx->d_whisk_draws, 0, ctx->cap_whisk_draws, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
  }
};
// the table's staging block holds k, the permutations and, after the chain, every blinder: both copies are zeroed before any return of a
// seeded entry (which set t->chain_used = 0 when it began)
hipError_t whisk_wipe_block(cg1_ctx* ctx, cg1_fixed* t) {
  const size_t used = std::min(t->chain_used, t->cap_chain);               // what this call's layouts reached
  if (!used) return hipSuccess;
  memset(t->h_chain, 0, used);
  const hipError_t e = hipMemsetAsync(t->d_chain, 0, used, ctx->stream), e2 = hipStreamSynchronize(ctx->stream);
  return e != hipSuccess ? e : e2;
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
  ShuffleWitness w{ell, n_provers, perm, {}};
  w.col[cg1whisk_host::COL_K] = k32; w.col[cg1whisk_host::COL_MBL] = vec_m_blinders32;
  return whisk_front(ctx, who, t, ell, n_provers, g_index, h_index, trackers96, w, out_rs_affine96, out_tu_affine96, out_post96, out_m48);
}

int cg1_whisk_shuffle_prove_device(cg1_ctx* ctx, cg1_fixed* t, size_t ell, size_t n_provers, const uint32_t* g_index, const uint32_t* h_index, const uint32_t* u_index,
                                   const uint32_t* gt_index, const uint32_t* gu_index, const uint8_t* gth_affine96, const uint8_t* trackers96, const uint32_t* perm,
                                   const uint8_t* k32, const uint8_t* vec_m_blinders32, const uint8_t* vec_a_blinders32, const uint8_t* vec_c_blinders32,
                                   const uint8_t* ipa_r32, const uint8_t* ipa_z_head32, const uint8_t* blinders32, const uint8_t* vec_r32, uint8_t* out_post96,
                                   uint8_t* out_proofs) {
  static const char* const who = "cg1_whisk_shuffle_prove_device";
  if (!ctx) return CG1_ERR_HIP;
  if (n_provers == 0) return CG1_OK;
  const bool pointers_ok = g_index && h_index && u_index && gt_index && gu_index && gth_affine96 && trackers96 && perm && k32 && vec_m_blinders32 && vec_a_blinders32 &&
                           vec_c_blinders32 && ipa_r32 && ipa_z_head32 && blinders32 && vec_r32 && out_post96 && out_proofs;
  if (!t || t->device != ctx->device || !pointers_ok) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", who); return CG1_ERR_ARG; }
  const ShuffleWitness w{ell, n_provers, perm, {k32, vec_m_blinders32, vec_a_blinders32, vec_c_blinders32, ipa_r32, ipa_z_head32, blinders32, vec_r32}};
  // both halves write into scratch of this call's; the caller's buffers are touched only when neither has refused.  (A shape or a P
  // the front refuses gets no scratch: the front refuses them before it writes.)
  const size_t P = n_provers, pts = cg1whisk_host::shape_ok(ell) && P <= CG1_SAME_MSM_MAX_PROVERS ? P * 2 * ell : 0;
  std::vector<uint8_t> rs(pts * 96), tu(pts * 96), post(pts * 48), m48(pts ? P * 48 : 0), proofs;
  if (const int rc = whisk_front(ctx, who, t, ell, P, g_index, h_index, trackers96, w, rs.data(), tu.data(), post.data(), m48.data())) return rc;
  proofs.resize(P * cg1_shuffle_prover_proof_bytes(ell));
  if (const int rc = shuffle_prove(ctx, who, t, ell, P, ShuffleCrsRows(g_index, h_index, u_index, gt_index, gu_index, gth_affine96), rs.data(), tu.data(), m48.data(), w, 1,
                                   proofs.data(), nullptr)) return rc;
  whisk_place_outputs(ell, P, nullptr, P, post.data(), m48.data(), proofs.data(), out_post96, out_proofs);
  return CG1_OK;
}

int cg1_whisk_shuffle_draws_device(cg1_ctx* ctx, size_t ell, size_t n_provers, const uint8_t* seed32, uint64_t first_index, uint32_t* out_perm, uint8_t* out_scalars32) {
  static const char* const who = "cg1_whisk_shuffle_draws_device";
  if (!ctx) return CG1_ERR_HIP;
  if (!seed32 || !out_perm || !out_scalars32) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", who); return CG1_ERR_ARG; }
  if (const int rc = cg1whisk_host::check_draws(ctx->err, sizeof ctx->err, who, ell, n_provers, first_index)) return rc;
  if (n_provers == 0) return CG1_OK;
  cg1::WipedBytes stage;
  if (const int rc = whisk_draws_run(ctx, ell, n_provers, seed32, first_index, stage)) return rc;
  const DrawBlock B = cg1whisk_host::draw_block(ell, n_provers);
  memcpy(out_perm, stage.v.data(), n_provers * ell * 4);
  memcpy(out_scalars32, stage.v.data() + (B.scalars - B.perm), B.total - B.scalars);
  return CG1_OK;
}

int cg1_whisk_shuffle_prove_seeded(cg1_ctx* ctx, cg1_fixed* t, size_t ell, size_t n_provers, const uint32_t* g_index, const uint32_t* h_index, const uint32_t* u_index,
                                   const uint32_t* gt_index, const uint32_t* gu_index, const uint8_t* gth_affine96, const uint8_t* trackers96, const uint8_t* seed32,
                                   uint64_t first_index, uint8_t* out_post96, uint8_t* out_proofs, int32_t* out_status, uint32_t* out_bad_at) {
  static const char* const who = "cg1_whisk_shuffle_prove_seeded";
  constexpr size_t NB = cg1whisk_host::N_BLINDERS;
  if (!ctx) return CG1_ERR_HIP;
  ctx->whisk_traffic[0] = ctx->whisk_traffic[1] = 0;
  if (n_provers == 0) return CG1_OK;
  const bool pointers_ok = g_index && h_index && u_index && gt_index && gu_index && gth_affine96 && trackers96 && seed32 && out_post96 && out_proofs && out_status && out_bad_at;
  if (!t || t->device != ctx->device || !pointers_ok) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", who); return CG1_ERR_ARG; }
  const size_t P = n_provers, n = ell + NB;
  if (const int rc = cg1whisk_host::check_shape(ctx->err, sizeof ctx->err, who, ell)) return rc;
  if (P > CG1_SAME_MSM_MAX_PROVERS || P * 2 * n > CG1_LIGHT_MAX_BASES) {
    snprintf(ctx->err, sizeof ctx->err, "%s: more than %d provers, or more than %d bases T | U, in one call", who, CG1_SAME_MSM_MAX_PROVERS, CG1_LIGHT_MAX_BASES);
    return CG1_ERR_ARG; }
  if (const int rc = cg1whisk_host::check_draws(ctx->err, sizeof ctx->err, who, ell, P, first_index)) return rc;
  if (const int rc = chain_check_indices(ctx, who, t, {{g_index, P * ell}, {h_index, P * NB}, {u_index, P}, {gt_index, P}, {gu_index, P}})) return rc;
  t->chain_used = 0;
  // ---- 1. the draws: on the device, and one copy down -- or, with "whisk_resident_witness", no copy: they stay where the kernels wrote
  // them until the guard zeroes them, and the front and the chain place them into their blocks on the device
  const bool resident = ctx->whisk_resident != 0;
  cg1::WipedBytes stage, kept;
  WhiskDrawsWipe wipe_draws(resident ? ctx : nullptr);
  if (const int rc = resident ? whisk_draws_enqueue(ctx, ell, P, seed32, first_index) : whisk_draws_run(ctx, ell, P, seed32, first_index, stage)) return rc;
  const ShuffleWitness drawn = resident ? ShuffleWitness::resident_draws((const uint8_t*)ctx->d_whisk_draws, ell, P) : ShuffleWitness::of_draws(stage.v.data(), ell, P);
  // ---- 2. the front, a status per prover
  const size_t pts = P * 2 * ell;
  std::vector<uint8_t> rs(pts * 96), tu(pts * 96), post(pts * 48), m48(P * 48), proofs, rs_kept, tu_kept, m_kept;
  std::vector<int32_t> st(P);
  std::vector<uint32_t> at(P);
  if (const int rc = whisk_front(ctx, who, t, ell, P, g_index, h_index, trackers96, drawn, rs.data(), tu.data(), post.data(), m48.data(), st.data(), at.data())) {
    (void)whisk_wipe_block(ctx, t); return rc; }
  // ---- 3. the provers it did not refuse, through the chain (its "prover" counts them, not the call's)
  std::vector<size_t> keep;
  for (size_t p = 0; p < P; ++p) if (!st[p]) keep.push_back(p);
  const size_t Q = keep.size();
  int rc = CG1_OK;
  const uint8_t* m_q = m48.data();                           // M of the kept provers, one after the other
  if (Q) {
    const ShuffleWitness w = drawn.gather(keep.data(), Q, kept);
    ctx->whisk_traffic[1] += kept.v.size();
    const ShuffleCrsRows crs(ShuffleCrsRows(g_index, h_index, u_index, gt_index, gu_index, gth_affine96), ell, P, keep.data(), Q);
    m_q = shuffle_rows(m48.data(), 48, P, keep.data(), Q, m_kept);
    proofs.resize(Q * cg1_shuffle_prover_proof_bytes(ell));
    rc = shuffle_prove(ctx, who, t, ell, Q, crs, shuffle_rows(rs.data(), 2 * ell * 96, P, keep.data(), Q, rs_kept), shuffle_rows(tu.data(), 2 * ell * 96, P, keep.data(), Q, tu_kept),
                       m_q, w, 1, proofs.data(), nullptr);
  }
  // ---- 4. secret hygiene (the draws' own device buffer and host staging: whisk_draws_run and WipedBytes, or WhiskDrawsWipe), then the caller's buffers
  const hipError_t wiped = whisk_wipe_block(ctx, t);
  if (rc) return rc;
  HIPCHK(wiped);
  whisk_place_outputs(ell, P, keep.data(), Q, post.data(), m_q, proofs.data(), out_post96, out_proofs);
  memcpy(out_status, st.data(), P * 4); memcpy(out_bad_at, at.data(), P * 4);
  return CG1_OK;
}

// What the last cg1_whisk_shuffle_prove_seeded call on this context moved of its witness: out[0] bytes copied device -> host, out[1] bytes
// the library wrote into host memory (the staging of the draws, the gathered rows, the block's witness fields, abl4).  Plain host counters
// beside those sites, zeroed when a seeded call begins; both are 0 after a call under "whisk_resident_witness" = 1.  The sites lie in
// whisk_front and shuffle_prove, which other entries share: read the counters straight after the seeded call, before any other.  For the tests.
void cg1_whisk_last_witness_traffic(const cg1_ctx* ctx, uint64_t out[2]) {
  out[0] = ctx ? ctx->whisk_traffic[0] : 0; out[1] = ctx ? ctx->whisk_traffic[1] : 0;
}
// 1 when every byte of the context's draws buffer is zero (or there is none), 0 when one is not, -1 on a HIP error.  One D2H copy.  For the tests.
int cg1_whisk_draws_buffer_is_zero(cg1_ctx* ctx) {
  if (!ctx) return -1;
  if (!ctx->d_whisk_draws || !ctx->cap_whisk_draws) return 1;
  std::vector<uint8_t> h(ctx->cap_whisk_draws);
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
      hipMemcpy(h.data(), ctx->d_whisk_draws, h.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  for (const uint8_t b : h) if (b) return 0;
  return 1;
}

// Host only, no HIP call: the front's (which_block = 0) or the chain's (1) staging block laid out exactly as the seeded entry lays it out
// for P drawn shuffles (the front) or for the Q of them keep[0] < .. < keep[Q - 1] names (the chain; keep == NULL: all P), with ONLY its
// witness fields filled, from draws_block (DrawBlock: swaps | perm | scalars, draw_block(ell, P).total bytes) -- resident = 0: by the
// copying path's own code, ShuffleWitness::gather and the stage functions over zero public inputs, of which only the witness fields are
// kept; resident = 1: by the placement map (place_source), as k_whisk_witness_place does.  -> the block's length, 0 for a shape or a
// keep list the entry would not reach; `out` (cap bytes) is written only when it holds the block, out_fields (2 words per field: offset,
// length) only up to *n_fields fields, and *n_fields becomes the number of witness fields.
size_t cg1_whisk_witness_block_emulate(size_t ell, size_t P, const size_t* keep, size_t Q, const uint8_t* draws_block, int resident, int which_block, uint8_t* out, size_t cap,
                                       uint64_t* out_fields, size_t* n_fields) {
  namespace W = cg1whisk_host;
  constexpr size_t NB = W::N_BLINDERS;
  const size_t n = ell + NB;
  if (!W::shape_ok(ell) || P < 1 || P > CG1_SAME_MSM_MAX_PROVERS || P * 2 * n > CG1_LIGHT_MAX_BASES || !draws_block || !n_fields || (which_block != 0 && which_block != 1)) return 0;
  std::vector<size_t> all(P);
  for (size_t p = 0; p < P; ++p) all[p] = p;
  if (which_block == 0 || !keep) { keep = all.data(); Q = P; }
  if (Q < 1 || Q > P) return 0;
  for (size_t q = 0; q < Q; ++q) if (keep[q] >= P || (q && keep[q] <= keep[q - 1])) return 0;
  // ---- the layouts, as whisk_front and shuffle_prove make them
  const WhiskLayout L = whisk_layout(ell, P);
  const ShuffleBlock blk = shuffle_block(ell, Q);
  const ShuffleLayout& SH = blk.SH;
  const SscalarLayout& SS = blk.SS;
  const GprodPlan& gp = blk.gp;
  const SmsmLayout& SM = blk.SM;
  const size_t total = which_block == 0 ? L.total : blk.total;
  size_t at[W::N_PLACE_FIELDS] = {0};
  whisk_front_place_at(at, L);
  shuffle_place_at(at, SH, SS, gp.L, SM);
  W::PlaceField f[W::N_PLACE_FIELDS];
  const size_t m = place_fields(which_block, -1, ell, P, at, f);
  for (size_t i = 0; out_fields && i < m && i < *n_fields; ++i) { out_fields[2 * i] = f[i].dst; out_fields[2 * i + 1] = (uint64_t)Q * f[i].dst_w * W::place_elem_bytes(f[i]); }
  *n_fields = m;
  if (!out || cap < total) return total;
  memset(out, 0, total);
  if (resident) {
    for (size_t i = 0; i < m; ++i) W::place_field_host(out, f[i], draws_block, ell, keep, Q);
    return total;
  }
  // ---- the copying path: the staging as it comes down, the gather, the stage functions into a block of its own
  const W::DrawBlock B = W::draw_block(ell, P);
  cg1::WipedBytes kept, block;
  block.v.assign(total, 0);
  const ShuffleWitness drawn = ShuffleWitness::of_draws(draws_block + B.perm, ell, P);
  const std::vector<uint32_t> zi(Q * n + 1, 0);
  if (which_block == 0) {
    (void)whisk_front_stage(block.v.data(), L, WhiskMFields{L.tb, L.sc, L.offs, L.m48, L.st_msm}, ell, P, zi.data(), zi.data(), drawn);
  } else {
    const ShuffleWitness w = drawn.gather(keep, Q, kept);
    const std::vector<uint8_t> zp(Q * 2 * n * 96 + cg1sscalar::SHARED_BASES * 96, 0), abl4 = shuffle_abl4(w);
    const SamePermHead sp{nullptr, nullptr, w.perm, abl4.data(), w.col[W::COL_MBL]};
    (void)shuffle_stage(block.v.data(), SH, SS, gp, SM, ell, Q, zi.data(), zi.data(), zi.data(), zp.data(), zp.data(), zp.data(), sp, w);
  }
  for (size_t i = 0; i < m; ++i) memcpy(out + f[i].dst, block.v.data() + f[i].dst, (size_t)Q * f[i].dst_w * W::place_elem_bytes(f[i]));
  return total;
}
}  // extern "C"
