// C ABI, part 15: a whole shuffle proof proved on the device -- CurdleProofsProof.new (curdleproofs.py:63-160) for n_provers shuffles of
// one ell in step, as ONE native call: k_shuffle_begin (kernels_shuffle.h) and the head MSMs A | A', then the parts of the same-scalar
// block (capi_same_scalar.h), the same-permutation chain (capi_gprod.h, capi_same_perm.h) and the same-MSM chain (capi_same_msm.h) on one
// stream, with the two transcript heads that need a device result run on the host behind an event each, under device work already queued.
// The entry is a pointer check in front of shuffle_prove, which the Whisk entries and the chain prover call under their own names with the
// witness as ONE value (ShuffleWitness, whisk_shuffle_host.h) and the CRS rows as another (ShuffleCrsRows).
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once
#include "whisk_shuffle_host.h"

namespace {
// the entry's own fields; the three arguments' layouts follow it in the block, behind the one states field
struct ShuffleLayout : ChainLayout {
  size_t perm, abl, gi_a, offs;                             // uploaded
  size_t pts, st_head;                                      // read back: A | A' per prover, the head launch's status
  size_t tb, sc;                                            // device only
};
ShuffleLayout shuffle_layout(size_t ell, size_t P, size_t base) {
  ShuffleLayout L{};
  L.begin(base);
  const size_t n = ell + cg1shuffle::N_BLINDERS;
  L.perm = L.take(P * ell * 4); L.abl = L.take(P * 2 * 32); L.gi_a = L.take(P * n * 4); L.offs = L.take((cg1shuffle::HEAD_MSMS * P + 1) * 4);
  L.up_end = L.total;
  L.down_begin = L.total;
  L.pts = L.take(P * cg1shuffle::HEAD_MSMS * 48); L.st_head = L.take(16);
  L.down_end = L.total;
  L.tb = L.take(P * cg1shuffle::head_terms((uint32_t)n) * 4); L.sc = L.take(P * cg1shuffle::head_terms((uint32_t)n) * 32);
  return L;
}
struct ShuffleEvents {                                      // the two host waits of a call
  hipEvent_t head = nullptr, mid = nullptr;
  ~ShuffleEvents() { if (head) (void)hipEventDestroy(head); if (mid) (void)hipEventDestroy(mid); }
};
// after a refusal that came down in mid-pipeline: nothing of the call may still be running when the block is laid out afresh
int shuffle_refuse(cg1_ctx* ctx, int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }

using cg1whisk_host::ShuffleWitness;
static_assert(cg1whisk_host::N_BLINDERS == cg1shuffle::N_BLINDERS, "the witness's column table is laid out for the prover's blinders");

// the rows keep[0 .. Q) of a table of P rows of `row` bytes, one after the other in `own`; all P rows: the table itself
const uint8_t* shuffle_rows(const uint8_t* all, size_t row, size_t P, const size_t* keep, size_t Q, std::vector<uint8_t>& own) {
  if (Q == P) return all;
  own.resize(Q * row);
  for (size_t q = 0; q < Q; ++q) memcpy(&own[q * row], all + keep[q] * row, row);
  return own.data();
}

// The CRS of P provers as index rows into the table: g (ell per prover), h (4), u, gt, gu (one each); gth_affine96 = G_t | G_u | H is the
// call's.  A view over the caller's rows, or over rows of its own: the rows a `keep` selects, or one row repeated.
struct ShuffleCrsRows {
  const uint32_t *g, *h, *u, *gt, *gu;
  const uint8_t* gth_affine96;
  ShuffleCrsRows(const uint32_t* g_, const uint32_t* h_, const uint32_t* u_, const uint32_t* gt_, const uint32_t* gu_, const uint8_t* gth)
      : g(g_), h(h_), u(u_), gt(gt_), gu(gu_), gth_affine96(gth) {}
  // the rows keep[0 .. Q) of `all`'s P (all P: `all` itself, and no copy); keep == NULL: row 0 of `all`, Q times
  ShuffleCrsRows(const ShuffleCrsRows& all, size_t ell, size_t P, const size_t* keep, size_t Q) : ShuffleCrsRows(all.g, all.h, all.u, all.gt, all.gu, all.gth_affine96) {
    constexpr size_t NB = cg1shuffle::N_BLINDERS;
    if (keep && Q == P) return;
    own.resize(Q * (ell + NB + 3));                         // g | h | u | gt | gu
    uint32_t* o = own.data();
    g = o; h = g + Q * ell; u = h + Q * NB; gt = u + Q; gu = gt + Q;
    for (size_t q = 0; q < Q; ++q) {
      const size_t p = keep ? keep[q] : 0;
      memcpy(o + q * ell, all.g + p * ell, ell * 4); memcpy(o + Q * ell + q * NB, all.h + p * NB, NB * 4);
      o[Q * (ell + NB) + q] = all.u[p]; o[Q * (ell + NB + 1) + q] = all.gt[p]; o[Q * (ell + NB + 2) + q] = all.gu[p];
    }
  }
  ShuffleCrsRows(const ShuffleCrsRows&) = delete;

 private:
  std::vector<uint32_t> own;
};

// The block of a whole shuffle for P provers: states | the entry's fields | same-scalar | same-permutation | same-MSM, laid end to end
// behind the one states field.  shuffle_prove lays its block out by this, and so does the host emulation of the witness's placement
// (cg1_whisk_witness_block_emulate): there is no second statement of the sequence.
struct ShuffleBlock {
  size_t states, pb_msm, total;
  ShuffleLayout SH;
  SscalarLayout SS;
  GprodPlan gp;
  SmsmLayout SM;
};
ShuffleBlock shuffle_block(size_t ell, size_t P) {
  const size_t n = ell + cg1shuffle::N_BLINDERS;
  ShuffleBlock B{};
  ChainLayout C{};
  B.states = C.take(P * 208);
  B.SH = shuffle_layout(ell, P, C.total);
  B.SS = sscalar_layout(ell, P, B.SH.total, B.states);
  B.gp = gprod_plan(ell, cg1shuffle::N_BLINDERS, P, true, B.SS.total, B.states);
  B.pb_msm = cg1_same_msm_proof_bytes(n);
  B.SM = smsm_layout(n, P, B.pb_msm, B.gp.L.total, B.states);
  B.total = B.SM.total;
  return B;
}

// ---- a resident witness (ShuffleWitness::resident): its fields are placed on the device, not staged.
// the fields of `block` that `phase` places (phase < 0: all of them), resolved for draws of draws_P provers; at[]: the fields' offsets in
// the block, by PlaceFieldId
size_t place_fields(int block, int phase, size_t ell, size_t draws_P, const size_t* at, cg1whisk_host::PlaceField* out) {
  namespace W = cg1whisk_host;
  size_t m = 0;
  for (int id = 0; id < W::N_PLACE_FIELDS; ++id) {
    const W::PlaceRule& r = W::PLACE_RULES[id];
    if (r.block == block && (phase < 0 || r.phase == phase)) out[m++] = W::place_resolve(r, ell, draws_P, at[id]);
  }
  return m;
}
// ... and ONE k_whisk_witness_place launch for them on the context's stream: behind the uploads that cover the fields (which carry whatever
// the host block held there) and in front of the first kernel that reads one
int whisk_place_enqueue(cg1_ctx* ctx, uint8_t* D, const ShuffleWitness& w, int block, int phase, const size_t* at) {
  namespace W = cg1whisk_host;
  W::PlaceField f[W::N_PLACE_FIELDS];
  cg1whisk::PlaceArgs a{};
  a.draws = w.d_draws; a.block = D; a.ell = (uint32_t)w.ell; a.Q = (uint32_t)w.P;
  a.n_fields = (uint32_t)place_fields(block, phase, w.ell, w.draws_P, at, f);
  if (a.n_fields > cg1whisk::PLACE_MAX_FIELDS || w.P > CG1_SAME_MSM_MAX_PROVERS) { snprintf(ctx->err, sizeof ctx->err, "the witness placement does not fit one launch"); return CG1_ERR_ARG; }
  for (size_t q = 0; q < w.P; ++q) a.keep[q] = (uint8_t)(w.keep ? w.keep[q] : q);
  uint32_t most = 1;
  for (uint32_t i = 0; i < a.n_fields; ++i) {
    a.f[i] = f[i];
    const uint32_t row = f[i].kind != W::PLACE_WORDS ? f[i].dst_w * 2u : (f[i].dst_w & 3u) ? f[i].dst_w : f[i].dst_w / 4u;      // lanes per row: the kernel's cut
    most = std::max(most, a.Q * row);
  }
  hipLaunchKernelGGL(cg1whisk::k_whisk_witness_place, dim3((most + cg1whisk::PLACE_THREADS - 1) / cg1whisk::PLACE_THREADS, a.n_fields), dim3(cg1whisk::PLACE_THREADS), 0,
                     ctx->stream, a);
  HIPCHK(hipGetLastError());
  return CG1_OK;
}

// The inputs of a whole shuffle into its block: the three arguments' (their *_stage functions) and the entry's own fields.  A resident
// witness leaves every witness field of the host block unwritten.  -> the witness bytes written into host memory: the lengths of the
// chain block's witness fields (place_bytes), which is what the copies below and in the *_stage functions write of it
size_t shuffle_stage(uint8_t* H, const ShuffleLayout& SH, const SscalarLayout& SS, const GprodPlan& gp, const SmsmLayout& SM, size_t ell, size_t P, const uint32_t* gi_a,
                     const uint32_t* gi_m, const uint32_t* u_index, const uint8_t* gth_affine96, const uint8_t* rs_affine96, const uint8_t* tu, const SamePermHead& sp,
                     const ShuffleWitness& w) {
  namespace W = cg1whisk_host;
  const size_t n = ell + cg1shuffle::N_BLINDERS;
  sscalar_stage(H, SS, ell, P, gth_affine96, rs_affine96, nullptr, w.col[W::COL_K], w.col[W::COL_BL]);
  gprod_stage(H, gp, gi_a, u_index, &sp, nullptr, nullptr, nullptr, w.col[W::COL_CBL], w.col[W::COL_IPA_R], w.col[W::COL_Z_HEAD]);
  smsm_stage(H, SM, n, P, gi_m, tu, nullptr, w.col[W::COL_VEC_R]);
  memcpy(H + SH.gi_a, gi_a, P * n * 4);
  if (w.resident()) return 0;
  memcpy(H + SH.perm, w.perm, P * ell * 4); memcpy(H + SH.abl, w.col[W::COL_ABL], P * 64);
  return W::place_bytes(W::BLOCK_CHAIN, ell, P);
}
// vec_a_blinders | 0 | 0 per prover, as the same-permutation head takes them (a host witness)
std::vector<uint8_t> shuffle_abl4(const ShuffleWitness& w) {
  constexpr size_t NB = cg1shuffle::N_BLINDERS;
  std::vector<uint8_t> abl4(w.P * NB * 32, 0);
  for (size_t p = 0; p < w.P; ++p) memcpy(&abl4[p * NB * 32], w.col[cg1whisk_host::COL_ABL] + p * 64, 64);
  return abl4;
}
void shuffle_place_at(size_t* at, const ShuffleLayout& SH, const SscalarLayout& SS, const GprodLayout& GP, const SmsmLayout& SM) {
  namespace W = cg1whisk_host;
  at[W::PF_SH_PERM] = SH.perm; at[W::PF_SH_ABL] = SH.abl; at[W::PF_SS_K] = SS.k; at[W::PF_SS_BL] = SS.bl;
  at[W::PF_GP_PERM] = GP.perm; at[W::PF_GP_ABL] = GP.abl; at[W::PF_GP_MBL] = GP.mbl; at[W::PF_GP_CBL] = GP.cbl; at[W::PF_GP_R] = GP.r; at[W::PF_GP_Z] = GP.z;
  at[W::PF_SM_VR] = SM.vr;
}

// The body of cg1_shuffle_prove_device, under the calling entry's name: the whole-shuffle entry, the Whisk entries (capi_whisk_shuffle.h)
// and the chain prover (capi_chain_prove.h) come here with pointers they have checked.  "prover p" in a refusal counts the P provers
// that reached this function.
int shuffle_prove(cg1_ctx* ctx, const char* who, cg1_fixed* t, size_t ell, size_t P, const ShuffleCrsRows& crs, const uint8_t* rs_affine96, const uint8_t* tu_affine96,
                  const uint8_t* m48, const ShuffleWitness& witness, int bases_certified, uint8_t* out_proofs, uint32_t* out_clocks) {
  namespace W = cg1whisk_host;
  static const char* const hashed_m[] = {"M"};
  constexpr size_t NB = cg1shuffle::N_BLINDERS;
  const uint32_t *g_index = crs.g, *h_index = crs.h, *u_index = crs.u, *gt_index = crs.gt, *gu_index = crs.gu, *perm = witness.perm;
  const uint8_t *gth_affine96 = crs.gth_affine96, *k32 = witness.col[W::COL_K], *vec_m_blinders32 = witness.col[W::COL_MBL],
                *vec_c_blinders32 = witness.col[W::COL_CBL], *ipa_r32 = witness.col[W::COL_IPA_R], *ipa_z_head32 = witness.col[W::COL_Z_HEAD],
                *blinders32 = witness.col[W::COL_BL], *vec_r32 = witness.col[W::COL_VEC_R];
  // ---- 1. refusals: the whole call, before anything is written -- the entry's own, then the three arguments' on what they will see
  const size_t n = ell + NB;
  const size_t pb = cg1_shuffle_prover_proof_bytes(ell);
  if (!pb) { snprintf(ctx->err, sizeof ctx->err, "%s: ell + %zu must be a power of two in 8 .. %d", who, NB, CG1_SAME_MSM_MAX_N); return CG1_ERR_ARG; }
  if (P > CG1_SAME_MSM_MAX_PROVERS || P * 2 * n > CG1_LIGHT_MAX_BASES) {
    snprintf(ctx->err, sizeof ctx->err, "%s: more than %d provers, or more than %d bases T | U, in one call", who, CG1_SAME_MSM_MAX_PROVERS, CG1_LIGHT_MAX_BASES);
    return CG1_ERR_ARG; }
  // what the arguments take: vec_G | vec_H and vec_G | vec_H[:2] | G_t | G_u as index rows, vec_a_blinders | 0 | 0, and the same-MSM
  // argument's vec_T | Z1 Z1 H Z1 | vec_U | Z1 Z1 Z1 H (the all-zero record is the identity)
  // A RESIDENT witness has no byte on the host: abl4 is not built, and every check below on a witness value is skipped (its list is
  // null, which the checks read as absent).  That is sound because such a witness is the device's own draws and nothing a caller stated:
  // every scalar left k_whisk_draws through fr_from_le64_wide, which reduces mod r, so it is canonical; k_whisk_fisher_yates swaps the
  // identity row in place, so each row is a permutation of 0 .. ell - 1 by construction; and the zero events (vec_c_blinders[2] == 0,
  // the second denominator) set the chains' device status bits as they do for a host witness -- ST_ZERO_C is checked here only to
  // refuse early.  Every check on a public input -- shape, indices, points -- stays.
  const bool resident = witness.resident();
  std::vector<uint32_t> gi_a(P * n), gi_m(P * n);
  std::vector<uint8_t> abl4, tu(P * 2 * n * 96, 0), canon_m(P * 48), tu48;
  if (!resident) { abl4 = shuffle_abl4(witness); ctx->whisk_traffic[1] += abl4.size(); }
  for (size_t p = 0; p < P; ++p) {
    memcpy(&gi_a[p * n], g_index + p * ell, ell * 4); memcpy(&gi_a[p * n + ell], h_index + p * NB, NB * 4);
    memcpy(&gi_m[p * n], g_index + p * ell, ell * 4); memcpy(&gi_m[p * n + ell], h_index + p * NB, 2 * 4);
    gi_m[p * n + ell + 2] = gt_index[p]; gi_m[p * n + ell + 3] = gu_index[p];
    uint8_t* T = &tu[p * 2 * n * 96];
    memcpy(T, tu_affine96 + p * 2 * ell * 96, ell * 96); memcpy(T + (ell + 2) * 96, gth_affine96 + 2 * 96, 96);
    memcpy(T + n * 96, tu_affine96 + (p * 2 * ell + ell) * 96, ell * 96); memcpy(T + (n + ell + 3) * 96, gth_affine96 + 2 * 96, 96);
  }
  const SamePermHead sp{nullptr, nullptr, perm, resident ? nullptr : abl4.data(), vec_m_blinders32};
  if (const int rc = gprod_check(ctx, who, same_perm_status_error, t, true, ell, NB, P, gi_a.data(), u_index, &sp, m48, 1, hashed_m, canon_m.data(), nullptr, nullptr,
                                 vec_c_blinders32, ipa_r32, ipa_z_head32)) return rc;
  if (const int rc = sscalar_check(ctx, who, t, true, ell, P, gth_affine96, rs_affine96, nullptr, k32, blinders32)) return rc;
  if (const int rc = smsm_check(ctx, who, t, true, n, P, gi_m.data(), nullptr, tu.data(), nullptr, vec_r32, nullptr, tu48)) return rc;
  // the 2 ell encodings of vec_R | vec_S per prover, for curdleproofs_step1 (vec_T | vec_U: in tu48)
  std::vector<uint8_t> rs48(P * 2 * ell * 48);
  {
    std::vector<uint8_t> blobs(P * 2 * ell * CG1_POINT_BYTES);
    for (size_t b = 0; b < P * 2 * ell; ++b) (void)cg1_from_affine96(&blobs[b * CG1_POINT_BYTES], rs_affine96 + 96 * b, 0);
    cg1_batch_compress(rs48.data(), blobs.data(), P * 2 * ell);
  }

  // ---- the block: states | the entry's fields | same-scalar | same-permutation | same-MSM, and everything a launch could otherwise
  // allocate in mid-chain
  ShuffleBlock blk = shuffle_block(ell, P);
  const size_t states = blk.states, pb_msm = blk.pb_msm;
  const ShuffleLayout& SH = blk.SH;
  const SscalarLayout& SS = blk.SS;
  GprodPlan& gp = blk.gp;
  const GprodLayout& GP = gp.L;
  const SmsmLayout& SM = blk.SM;
  uint8_t* H; uint8_t* D;
  if (const int rc = chain_reserve(ctx, t, SM.total, H, D)) return rc;
  const size_t bases_rs = cg1sscalar::SHARED_BASES + P * 2 * ell, bases_tu = P * 2 * n;
  cg1_light* lt;
  if (const int rc = chain_light_scratch(ctx, t, std::max(bases_rs, bases_tu), lt)) return rc;
  const uint32_t Pn = (uint32_t)P, nn = (uint32_t)n, M0 = cg1shuffle::HEAD_MSMS * Pn;
  const TableShape shape0 = table_pick_shape<FixedKind>(ctx, M0, nn);
  TableShape shape_ss;
  {
    const size_t S = (nn + shape0.slice - 1) / shape0.slice, need = S > 1 ? (size_t)M0 * S : 0;
    if (const int rc = cg1::grow_device(ctx, t->d_partial, t->cap_partial, need, need)) return rc;
  }
  if (const int rc = gprod_reserve(ctx, t, gp)) return rc;
  if (const int rc = sscalar_reserve(ctx, lt, ell, P, shape_ss)) return rc;
  if (const int rc = smsm_reserve(ctx, t, lt, n, P)) return rc;
  ShuffleEvents ev;
  HIPCHK(hipEventCreateWithFlags(&ev.head, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&ev.mid, hipEventDisableTiming));

  // ---- 2. the head on the host, per prover: curdleproofs_step1 [vec_R + vec_S + vec_T + vec_U], M, curdleproofs_vec_a x ell
  chain_clear(H, SS, P); chain_clear(H, GP, P); chain_clear(H, SM, P);
  ctx->whisk_traffic[1] += shuffle_stage(H, SH, SS, gp, SM, ell, P, gi_a.data(), gi_m.data(), u_index, gth_affine96, rs_affine96, tu.data(), sp, witness);
  size_t place_at[W::N_PLACE_FIELDS] = {0};
  shuffle_place_at(place_at, SH, SS, GP, SM);
  for (uint32_t p = 0; p < Pn; ++p) cg1shuffle::head_offsets(nn, p * cg1shuffle::head_terms(nn), reinterpret_cast<uint32_t*>(H + SH.offs) + cg1shuffle::HEAD_MSMS * p);
  cg1::pool_for(P, 0, [&](size_t p) {
    static const uint8_t label[] = "curdleproofs", step1[] = "curdleproofs_step1", l_a[] = "curdleproofs_vec_a";
    uint8_t* st = H + states + 208 * p;
    std::vector<uint8_t> list(4 * ell * 48);
    memcpy(&list[0], &rs48[p * 2 * ell * 48], 2 * ell * 48);
    memcpy(&list[2 * ell * 48], &tu48[p * 2 * n * 48], ell * 48);
    memcpy(&list[3 * ell * 48], &tu48[(p * 2 * n + n) * 48], ell * 48);
    cg1_merlin_init(st, label, 12);
    cg1_merlin_append_list(st, step1, 18, list.data(), 48, 4 * ell);
    cg1_merlin_append(st, step1, 18, &canon_m[48 * p], 48);
    for (size_t i = 0; i < ell; ++i) cg1_merlin_challenge_scalar(st, l_a, 18, H + SS.va + (p * ell + i) * 32);
  });
  if (const int rc = chain_upload(ctx, t, SH)) return rc;
  if (const int rc = chain_upload(ctx, t, SS)) return rc;
  if (const int rc = chain_upload(ctx, t, SM)) return rc;     // (its vx field goes up as it lies: k_shuffle_begin writes it next)
  if (resident) { if (const int rc = whisk_place_enqueue(ctx, D, witness, W::BLOCK_CHAIN, 0, place_at)) return shuffle_refuse(ctx, rc); }

  // ---- 3, 4. k_shuffle_begin, then A | A' as one launch over the CRS table; their encodings come down behind the first event
  lt->n_bases = bases_rs;
  const cg1sscalar::SscalarArgs ssa = sscalar_args(D, SS, ell, lt, bases_certified);
  const cg1smsm::SmsmArgs sma = smsm_args(D, SM, n, pb_msm, t, lt);
  {
    cg1shuffle::ShuffleBeginArgs b;
    b.ell = (uint32_t)ell;
    b.va = ssa.va; b.perm = (const uint32_t*)(D + SH.perm); b.k = ssa.k; b.bl = ssa.bl; b.abl = (const uint64_t*)(D + SH.abl);
    b.gi_a = (const uint32_t*)(D + SH.gi_a); b.gi_m = sma.gi;
    b.tb = (uint32_t*)(D + SH.tb); b.sc = (uint64_t*)(D + SH.sc); b.vx = (uint64_t*)(D + SM.vx);
    b.ss_tb = ssa.tb; b.ss_sc = ssa.sc;
    hipLaunchKernelGGL(cg1shuffle::k_shuffle_begin, dim3(Pn), dim3(cg1shuffle::SH_THREADS), 0, ctx->stream, b);
    if (const int rc = table_enqueue<FixedKind>(ctx, t, b.tb, (const uint32_t*)b.sc, (const uint32_t*)(D + SH.offs), M0, Pn * cg1shuffle::head_terms(nn), nn, shape0, false,
                                                nullptr, D + SH.pts)) return shuffle_refuse(ctx, rc);
  }
  HIPCHK(hipMemcpyAsync(D + SH.st_head, t->d_status, 16, hipMemcpyDeviceToDevice, ctx->stream));
  if (const int rc = chain_download(ctx, t, SH)) return shuffle_refuse(ctx, rc);
  HIPCHK(hipEventRecord(ev.head, ctx->stream));

  // ---- 5. behind it, without waiting: the same-scalar block's table and its ten MSMs per prover (k_shuffle_begin wrote their terms)
  if (const int rc = sscalar_enqueue_msms(ctx, lt, D, SS, ssa, ell, P, bases_certified, shape_ss)) return shuffle_refuse(ctx, rc);

  // ---- 6. the first wait; the same-permutation head on the host, under step 5, then its chain
  HIPCHK(hipEventSynchronize(ev.head));
  if (const int rc = table_status_error<FixedKind>(ctx, reinterpret_cast<const uint32_t*>(H + SH.st_head)[0])) return shuffle_refuse(ctx, rc);
  cg1::pool_for(P, 0, [&](size_t p) {
    uint8_t am[96];
    memcpy(am, H + SH.pts + p * 96, 48); memcpy(am + 48, &canon_m[48 * p], 48);
    same_perm_head(H, gp, p, am, H + SS.va + p * ell * 32);
  });
  HIPCHK(hipMemcpyAsync(D + states, H + states, P * 208, hipMemcpyHostToDevice, ctx->stream));
  if (const int rc = chain_upload(ctx, t, GP)) return shuffle_refuse(ctx, rc);
  if (resident) { if (const int rc = whisk_place_enqueue(ctx, D, witness, W::BLOCK_CHAIN, 1, place_at)) return shuffle_refuse(ctx, rc); }
  const cg1sperm::SamePermArgs spa = gprod_args(ctx, t, D, gp, true);
  if (const int rc = gprod_enqueue(ctx, t, D, gp, spa, true)) return shuffle_refuse(ctx, rc);

  // ---- 7. the same-scalar block's step on the states the same-permutation chain left; both arguments come down behind the second event
  hipLaunchKernelGGL(cg1sscalar::k_sscalar_step, dim3(Pn), dim3(cg1sscalar::SS_THREADS), 0, ctx->stream, ssa, cg1sscalar::SS_STEP);
  HIPCHK(hipMemcpyAsync(H + states, D + states, P * 208, hipMemcpyDeviceToHost, ctx->stream));
  if (const int rc = chain_download(ctx, t, GP)) return shuffle_refuse(ctx, rc);
  if (const int rc = chain_download(ctx, t, SS)) return shuffle_refuse(ctx, rc);
  HIPCHK(hipEventRecord(ev.mid, ctx->stream));

  // ---- 8. behind it, without waiting: the same-MSM chain's begin and its table over T | U, into the scratch the R | S table has left
  lt->n_bases = bases_tu;
  smsm_enqueue_begin(ctx, lt, D, SM, sma, n, P);

  // ---- 9. the second wait; same_msm_step1 [A', Z_t, Z_u] and the 2 n encodings on the host, under step 8, then the rest of the chain
  HIPCHK(hipEventSynchronize(ev.mid));
  if (const int rc = chain_status_error(ctx, H, GP, who, same_perm_status_error)) return shuffle_refuse(ctx, rc);
  if (const int rc = chain_status_error(ctx, H, SS, who, same_scalar_status_error)) return shuffle_refuse(ctx, rc);
  cg1::pool_for(P, 0, [&](size_t p) {
    const uint8_t* ss = H + SS.proof + p * cg1sscalar::PROOF_BYTES;         // cm_T = T_1 | T_2, cm_U = U_1 | U_2, ...
    uint8_t head[144];
    memcpy(head, H + SH.pts + p * 96 + 48, 48); memcpy(head + 48, ss + 48, 48); memcpy(head + 96, ss + 144, 48);
    smsm_absorb(H + states + 208 * p, head, &tu48[p * 2 * n * 48], n);
  });
  HIPCHK(hipMemcpyAsync(D + states, H + states, P * 208, hipMemcpyHostToDevice, ctx->stream));
  if (const int rc = smsm_enqueue_rounds(ctx, t, lt, D, SM, sma, n, P)) return shuffle_refuse(ctx, rc);

  // ---- 10. the last copy down, the stream wait, and only then the caller's buffers
  if (const int rc = chain_download(ctx, t, SM)) return shuffle_refuse(ctx, rc);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  if (const int rc = chain_status_error(ctx, H, SM, who, nullptr)) return rc;
  const size_t pb_perm = gp.pb;
  for (size_t p = 0; p < P; ++p) {                          // A | cm_T | cm_U | R | S | same_perm | cm_A | cm_B | z_k | z_t | z_u | same_msm
    uint8_t* out = out_proofs + p * pb;
    const uint8_t* ss = H + SS.proof + p * cg1sscalar::PROOF_BYTES;
    memcpy(out, H + SH.pts + p * 96, 48);
    memcpy(out + 48, ss, 288);
    memcpy(out + 336, H + GP.proof + p * pb_perm, pb_perm);
    memcpy(out + 336 + pb_perm, ss + 288, 288);
    memcpy(out + 624 + pb_perm, H + SM.proof + p * pb_msm, pb_msm);
  }
  if (out_clocks)                                           // the three chains' clock words, summed
    for (size_t i = 0; i < P * 4; ++i)
      out_clocks[i] = reinterpret_cast<const uint32_t*>(H + SS.clocks)[i] + reinterpret_cast<const uint32_t*>(H + GP.clocks)[i] + reinterpret_cast<const uint32_t*>(H + SM.clocks)[i];
  return CG1_OK;
}
}  // namespace

extern "C" {
size_t cg1_shuffle_prover_proof_bytes(size_t ell) {
  const size_t n = ell + cg1shuffle::N_BLINDERS;
  if (ell < 1 || n < ell || !chain_pow2(n) || n > CG1_SAME_MSM_MAX_N) return 0;
  return 48 + 288 + cg1_same_perm_proof_bytes(ell, cg1shuffle::N_BLINDERS) + 288 + cg1_same_msm_proof_bytes(n);
}

int cg1_shuffle_prove_device(cg1_ctx* ctx, cg1_fixed* t, size_t ell, size_t n_provers, const uint32_t* g_index, const uint32_t* h_index, const uint32_t* u_index,
                             const uint32_t* gt_index, const uint32_t* gu_index, const uint8_t* gth_affine96, const uint8_t* rs_affine96, const uint8_t* tu_affine96,
                             const uint8_t* m48, const uint32_t* perm, const uint8_t* k32, const uint8_t* vec_m_blinders32, const uint8_t* vec_a_blinders32,
                             const uint8_t* vec_c_blinders32, const uint8_t* ipa_r32, const uint8_t* ipa_z_head32, const uint8_t* blinders32, const uint8_t* vec_r32,
                             int bases_certified, uint8_t* out_proofs, uint32_t* out_clocks) {
  static const char* const who = "cg1_shuffle_prove_device";
  if (!ctx) return CG1_ERR_HIP;
  if (n_provers == 0) return CG1_OK;
  const bool pointers_ok = g_index && h_index && u_index && gt_index && gu_index && gth_affine96 && rs_affine96 && tu_affine96 && m48 && perm && k32 &&
                           vec_m_blinders32 && vec_a_blinders32 && vec_c_blinders32 && ipa_r32 && ipa_z_head32 && blinders32 && vec_r32 && out_proofs;
  if (!t || t->device != ctx->device || !pointers_ok) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", who); return CG1_ERR_ARG; }
  const ShuffleWitness w{ell, n_provers, perm, {k32, vec_m_blinders32, vec_a_blinders32, vec_c_blinders32, ipa_r32, ipa_z_head32, blinders32, vec_r32}};
  return shuffle_prove(ctx, who, t, ell, n_provers, ShuffleCrsRows(g_index, h_index, u_index, gt_index, gu_index, gth_affine96), rs_affine96, tu_affine96, m48, w,
                       bases_certified, out_proofs, out_clocks);
}
}  // extern "C"
