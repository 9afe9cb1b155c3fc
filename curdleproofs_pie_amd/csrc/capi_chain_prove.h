// C ABI, part 23: a chain of Whisk shuffles PROVED over the device-resident tracker set (shuffle_chain.py: ShuffleChainProver,
// TrackerSet.evolve).  Block j reads pre_j = [set[i] for i in indices_j] before any of its own writes and writes set[indices_j[t]] =
// k_j * pre_j[perm_j[t]]; the dependence between blocks lies in the trackers alone, so the trackers of ALL blocks are made first --
//   certify   the distinct slots the call reads at first touch: k_chain_gather of their records aside, k_subgroup_row, one copy down, the
//             first wait (the set's records are decoded unchecked, and the chain verifier may have scattered posts outside G1 into it)
//   lineage   cg1chain::lineage (chain_lineage.h, host): a status per block, (origin slot, composite scalar) per position, the last writers
//   multiply  k_chain_lineage_mul (kernels_chain_prove.h): ONE launch without dependencies -> vec_R | vec_S, vec_T | vec_U, T_t | U_t
//   advance   k_chain_scatter of the last writers' records, with zero status bytes, into the set
// -- and the proofs, independent now, go through shuffle_prove (capi_shuffle.h) in groups of CG1_SAME_MSM_MAX_PROVERS with M by whisk_m_run.
//   cg1_chain_evolve_device   the tracker stage alone, permutations and scalars the caller's
//   cg1_chain_prove_seeded    the draws of cg1_whisk_shuffle_prove_seeded for all blocks (kept in wiped host staging: D 32 bytes per block),
//                             the tracker stage, the proofs
// Neither entry restores the set when it fails behind the advance: the caller holds the host bytes and decodes them afresh.
// Part of the single translation unit csrc/msm_gpu.hip (behind capi_whisk_shuffle.h and capi_tracker_set.h).
#pragma once
#include "chain_lineage.h"

namespace {
struct ChainStageOut {
  std::vector<int32_t> status;
  std::vector<uint32_t> bad_at, writers;                   // writers: (slot, b ell + t) pairs
  size_t n_writers = 0, certified_slots = 0;
  std::vector<uint8_t> rs, tu, post;                       // [n][2][ell] x 96 (records only when asked for), [n][ell][2] x 48; zeros for a refused block
  float ms = 0.f;                                          // the stage between two events on the stream
};

// ctx->d_chain_prove, laid out afresh by every call
struct ChainStageLayout { size_t plan, cpts, cstat, cflags, origin, scalar, rs, tu, post, zstat, total; };
ChainStageLayout chain_stage_layout(size_t m2, size_t pos) {       // m2: certified points, pos: n 2 ell positions
  ChainStageLayout L{};
  size_t at = 0;
  auto take = [&](size_t b) { const size_t o = at; at = (at + b + 255) & ~(size_t)255; return o; };
  L.plan = take(m2 * 4); L.cpts = take(m2 * 96); L.cstat = take(m2); L.cflags = take(m2);
  L.origin = take(pos * 4); L.scalar = take(pos * 32);
  L.rs = take(pos * 96); L.tu = take(pos * 96); L.post = take(pos * 48); L.zstat = take(pos);
  L.total = at;
  return L;
}

// The tracker stage on the context's stream; indices, perm and k32 have passed cg1chain::lineage_check.  Two waits: behind the
// certification and behind the last copy down.  The origins (which spell the permutations out) and the composites leave no trace: their
// device fields are zeroed, their host staging wiped.
int chain_tracker_stage(cg1_ctx* ctx, const char* who, void* d_set_pts96, void* d_set_pstat, size_t n_slots, const uint32_t* indices, const uint32_t* perm,
                        const uint8_t* k32, size_t n, size_t ell, bool want_records, ChainStageOut& out) {
  const size_t pos = n * 2 * ell;
  // ---- the distinct slots, in order of first touch
  std::vector<uint32_t> slots;
  {
    std::vector<bool> seen(n_slots, false);
    for (size_t e = 0; e < n * ell; ++e)
      if (!seen[indices[e]]) { seen[indices[e]] = true; slots.push_back(indices[e]); }
  }
  const size_t m2 = 2 * slots.size();
  out.certified_slots = slots.size();
  const ChainStageLayout L = chain_stage_layout(m2, pos);
  HIPCHK(hipSetDevice(ctx->device));
  if (const int rc = cg1::grow_bufs(ctx, ctx->cap_chain_prove, L.total, L.total, {cg1::dev_buf(ctx->d_chain_prove, L.total)})) return rc;
  uint8_t* D = (uint8_t*)ctx->d_chain_prove;
  hipEvent_t ev[2] = {nullptr, nullptr};
  HIPCHK(hipEventCreate(&ev[0]));
  if (hipEventCreate(&ev[1]) != hipSuccess) { (void)hipEventDestroy(ev[0]); snprintf(ctx->err, sizeof ctx->err, "%s: hipEventCreate failed", who); return CG1_ERR_HIP; }
  struct Events { hipEvent_t* e; ~Events() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); } } events{ev};
  HIPCHK(hipEventRecord(ev[0], ctx->stream));
  // ---- certify
  std::vector<int32_t> plan(m2);
  for (size_t i = 0; i < slots.size(); ++i) { plan[2 * i] = ~(int32_t)(2 * slots[i]); plan[2 * i + 1] = ~(int32_t)(2 * slots[i] + 1); }
  std::vector<uint8_t> cert(2 * m2);                       // the records' status bytes, then the subgroup flags
  HIPCHK(hipMemcpyAsync(D + L.plan, plan.data(), m2 * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(cg1::k_chain_gather, dim3((unsigned)((m2 * 8 + 255) / 256)), dim3(256), 0, ctx->stream, (uint4*)(D + L.cpts), D + L.cstat, (uint32_t)m2,
                     (const uint4*)d_set_pts96, (const uint8_t*)d_set_pstat, (uint32_t)(2 * n_slots), (const int32_t*)(D + L.plan), 0u, 1u, (uint32_t)m2, (uint32_t)m2);
  hipLaunchKernelGGL(cg1::k_subgroup_row, dim3((unsigned)m2), dim3(64), 0, ctx->stream, (const uint32_t*)(D + L.cpts), (uint32_t)m2, D + L.cflags);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(cert.data(), D + L.cstat, m2, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(cert.data() + m2, D + L.cflags, m2, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));               // the first wait
  std::vector<uint8_t> point_status(2 * n_slots, 0);
  for (size_t i = 0; i < slots.size(); ++i)
    for (size_t half = 0; half < 2; ++half)
      point_status[2 * (size_t)slots[i] + half] = cert[2 * i + half] ? CG1_WHISK_SHUFFLE_NO_DECODE : cert[m2 + 2 * i + half] ? 0 : CG1_WHISK_SHUFFLE_NOT_G1;
  // ---- lineage
  out.status.assign(n, 0); out.bad_at.assign(n, 0);
  out.writers.assign(2 * std::min(n_slots, n * ell), 0);
  cg1::WipedBytes lin;                                      // origins (they spell the permutations out) | composites
  lin.v.resize(pos * 36);
  uint32_t* origin = reinterpret_cast<uint32_t*>(lin.v.data());
  uint8_t* comp = lin.v.data() + pos * 4;
  if (const int rc = cg1chain::lineage(n_slots, point_status.data(), indices, perm, k32, n, ell, out.status.data(), out.bad_at.data(), origin, comp,
                                       out.writers.data(), &out.n_writers)) { snprintf(ctx->err, sizeof ctx->err, "%s: the lineage refused its flags", who); return rc; }
  // ---- multiply, advance, one copy down
  out.post.assign(pos * 48, 0);
  if (want_records) { out.rs.assign(pos * 96, 0); out.tu.assign(pos * 96, 0); }
  std::vector<uint32_t> pairs(4 * out.n_writers);          // set point <- point of vec_T | vec_U
  for (size_t w = 0; w < out.n_writers; ++w) {
    const size_t slot = out.writers[2 * w], b = out.writers[2 * w + 1] / ell, t = out.writers[2 * w + 1] % ell;
    for (size_t half = 0; half < 2; ++half) {
      pairs[4 * w + 2 * half] = (uint32_t)(2 * slot + half);
      pairs[4 * w + 2 * half + 1] = (uint32_t)(b * 2 * ell + half * ell + t);
    }
  }
  auto run = [&]() -> int {
    HIPCHK(hipMemcpyAsync(D + L.origin, origin, pos * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(D + L.scalar, comp, pos * 32, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(D + L.zstat, 0, pos, ctx->stream));
    cg1whisk::LineageMulArgs a;
    a.ell = (uint32_t)ell; a.n_blocks = (uint32_t)n; a.n_set_points = (uint32_t)(2 * n_slots);
    a.set96 = (const uint32_t*)d_set_pts96; a.origin = (const uint32_t*)(D + L.origin); a.scalar = (const uint32_t*)(D + L.scalar);
    a.rs96 = (uint32_t*)(D + L.rs); a.tu96 = (uint32_t*)(D + L.tu); a.post48 = (uint32_t*)(D + L.post);
    hipLaunchKernelGGL(cg1whisk::k_chain_lineage_mul, dim3((unsigned)(2 * pos)), dim3(64), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    if (const int rc = cg1_chain_scatter_enqueue(ctx, D + L.tu, D + L.zstat, pos, d_set_pts96, d_set_pstat, 2 * n_slots, pairs.data(), 2 * out.n_writers)) return rc;
    HIPCHK(hipMemcpyAsync(out.post.data(), D + L.post, pos * 48, hipMemcpyDeviceToHost, ctx->stream));
    if (want_records) {
      HIPCHK(hipMemcpyAsync(out.rs.data(), D + L.rs, pos * 96, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipMemcpyAsync(out.tu.data(), D + L.tu, pos * 96, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipEventRecord(ev[1], ctx->stream));
    return CG1_OK;
  };
  const int rc = run();
  const hipError_t w1 = hipMemsetAsync(D + L.origin, 0, L.rs - L.origin, ctx->stream), w2 = hipStreamSynchronize(ctx->stream);      // whatever run() said
  if (rc) return rc;
  HIPCHK(w1); HIPCHK(w2);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventElapsedTime(&out.ms, ev[0], ev[1]));
  for (size_t b = 0; b < n; ++b) {                         // the kernel wrote nothing for a refused block: the field holds an earlier call's bytes there
    if (!out.status[b]) continue;
    memset(&out.post[b * 2 * ell * 48], 0, 2 * ell * 48);
    if (want_records) { memset(&out.rs[b * 2 * ell * 96], 0, 2 * ell * 96); memset(&out.tu[b * 2 * ell * 96], 0, 2 * ell * 96); }
  }
  return CG1_OK;
}

int chain_stage_args(cg1_ctx* ctx, const char* who, const void* d_set_pts96, const void* d_set_pstat, size_t n_slots) {
  if (!d_set_pts96 || !d_set_pstat || ((uintptr_t)d_set_pts96 & 15) || n_slots == 0 || n_slots >= (1ull << 30)) {
    snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", who);
    return CG1_ERR_ARG; }
  return CG1_OK;
}
}  // namespace

extern "C" {
int cg1_chain_evolve_device(cg1_ctx* ctx, void* d_set_pts96, void* d_set_pstat, size_t n_slots, const uint32_t* indices, const uint32_t* perm, const uint8_t* k32,
                            size_t n_blocks, size_t ell, uint8_t* out_post96, int32_t* out_status, uint32_t* out_bad_at, uint32_t* out_writers, size_t* out_n_writers,
                            float* out_stats) {
  static const char* const who = "cg1_chain_evolve_device";
  if (!ctx) return CG1_ERR_HIP;
  if (out_n_writers) *out_n_writers = 0;
  if (n_blocks == 0) return CG1_OK;
  if (!indices || !perm || !k32 || !out_post96 || !out_status || !out_bad_at || !out_writers || !out_n_writers) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", who); return CG1_ERR_ARG; }
  if (const int rc = chain_stage_args(ctx, who, d_set_pts96, d_set_pstat, n_slots)) return rc;
  if (const int rc = cg1chain::lineage_check(ctx->err, sizeof ctx->err, who, n_slots, indices, perm, k32, n_blocks, ell)) return rc;
  ChainStageOut S;
  if (const int rc = chain_tracker_stage(ctx, who, d_set_pts96, d_set_pstat, n_slots, indices, perm, k32, n_blocks, ell, false, S)) return rc;
  memcpy(out_post96, S.post.data(), S.post.size());
  memcpy(out_status, S.status.data(), n_blocks * 4); memcpy(out_bad_at, S.bad_at.data(), n_blocks * 4);
  memcpy(out_writers, S.writers.data(), S.n_writers * 8);
  *out_n_writers = S.n_writers;
  if (out_stats) { out_stats[0] = S.ms; out_stats[1] = (float)S.certified_slots; }
  return CG1_OK;
}

int cg1_chain_prove_seeded(cg1_ctx* ctx, cg1_fixed* t, size_t ell, size_t n_blocks, const uint32_t* g_index, const uint32_t* h_index, uint32_t u_index, uint32_t gt_index,
                           uint32_t gu_index, const uint8_t* gth_affine96, void* d_set_pts96, void* d_set_pstat, size_t n_slots, const uint32_t* indices,
                           const uint8_t* seed32, uint64_t first_index, uint8_t* out_post96, uint8_t* out_proofs, int32_t* out_status, uint32_t* out_bad_at,
                           uint32_t* out_writers, size_t* out_n_writers, float* out_stats) {
  static const char* const who = "cg1_chain_prove_seeded";
  constexpr size_t NB = cg1whisk_host::N_BLINDERS;
  if (!ctx) return CG1_ERR_HIP;
  if (out_n_writers) *out_n_writers = 0;
  if (n_blocks == 0) return CG1_OK;
  const bool pointers_ok = g_index && h_index && gth_affine96 && indices && seed32 && out_post96 && out_proofs && out_status && out_bad_at && out_writers && out_n_writers;
  if (!t || t->device != ctx->device || !pointers_ok) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", who); return CG1_ERR_ARG; }
  if (const int rc = chain_stage_args(ctx, who, d_set_pts96, d_set_pstat, n_slots)) return rc;
  const size_t N = n_blocks, n = ell + NB;
  if (const int rc = cg1whisk_host::check_draws(ctx->err, sizeof ctx->err, who, ell, N, first_index)) return rc;
  const size_t G = std::min<size_t>(CG1_SAME_MSM_MAX_PROVERS, CG1_LIGHT_MAX_BASES / (2 * n));       // provers per group
  if (G == 0) { snprintf(ctx->err, sizeof ctx->err, "%s: more than %d bases T | U in one shuffle", who, CG1_LIGHT_MAX_BASES); return CG1_ERR_ARG; }
  const uint32_t one_each[3] = {u_index, gt_index, gu_index};
  if (const int rc = chain_check_indices(ctx, who, t, {{g_index, ell}, {h_index, NB}, {one_each, 3}})) return rc;
  for (size_t e = 0; e < N * ell; ++e)
    if (indices[e] >= n_slots) { snprintf(ctx->err, sizeof ctx->err, "%s: block %zu: a slot index outside the set", who, e / ell); return CG1_ERR_ARG; }
  const auto wall = [] { return std::chrono::steady_clock::now(); };
  const auto ms_since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - a).count(); };
  const auto t_call = wall();
  t->chain_used = 0;
  // ---- 1. the draws of all blocks: on the device, one copy down, kept in wiped host staging
  cg1::WipedBytes stage;
  if (const int rc = whisk_draws_run(ctx, ell, N, seed32, first_index, stage)) return rc;
  const ShuffleWitness drawn = ShuffleWitness::of_draws(stage.v.data(), ell, N);
  const uint8_t* k32 = drawn.col[cg1whisk_host::COL_K];
  if (const int rc = cg1chain::lineage_check(ctx->err, sizeof ctx->err, who, n_slots, indices, drawn.perm, k32, N, ell)) return rc;
  // ---- 2. the trackers of every block, the set advanced
  ChainStageOut S;
  if (const int rc = chain_tracker_stage(ctx, who, d_set_pts96, d_set_pstat, n_slots, indices, drawn.perm, k32, N, ell, true, S)) return rc;
  // ---- 3. the proofs: the surviving blocks in groups, each M by one table launch and then the whole-shuffle chain, bases certified (its
  // "prover" counts the blocks of the group)
  const size_t pb = cg1_shuffle_prover_proof_bytes(ell);
  std::vector<size_t> keep;
  for (size_t b = 0; b < N; ++b) if (!S.status[b]) keep.push_back(b);
  std::vector<uint8_t> all_m(keep.size() * 48), all_proofs(keep.size() * pb);
  float ms_chain = 0.f;
  int rc = CG1_OK;
  for (size_t lo = 0; lo < keep.size() && !rc; lo += G) {
    const size_t Q = std::min(G, keep.size() - lo);
    cg1::WipedBytes kept;
    const ShuffleWitness w = drawn.gather(&keep[lo], Q, kept);
    const ShuffleCrsRows crs(ShuffleCrsRows(g_index, h_index, one_each, one_each + 1, one_each + 2, gth_affine96), ell, 1, nullptr, Q);      // the one CRS, Q times
    std::vector<uint8_t> rs_kept, tu_kept;
    const uint8_t* rs = shuffle_rows(S.rs.data(), 2 * ell * 96, N, &keep[lo], Q, rs_kept);
    const uint8_t* tu = shuffle_rows(S.tu.data(), 2 * ell * 96, N, &keep[lo], Q, tu_kept);
    if ((rc = whisk_m_run(ctx, who, t, ell, Q, crs, w, &all_m[lo * 48]))) break;
    const auto t_chain = wall();
    rc = shuffle_prove(ctx, who, t, ell, Q, crs, rs, tu, &all_m[lo * 48], w, 1, &all_proofs[lo * pb], nullptr);
    ms_chain += ms_since(t_chain);
  }
  // ---- 4. secret hygiene (the draws and composites: whisk_draws_run, chain_tracker_stage, WipedBytes), then the caller's buffers
  const hipError_t wiped = whisk_wipe_block(ctx, t);
  if (rc) return rc;
  HIPCHK(wiped);
  whisk_place_outputs(ell, N, keep.data(), keep.size(), S.post.data(), all_m.data(), all_proofs.data(), out_post96, out_proofs);
  memcpy(out_status, S.status.data(), N * 4); memcpy(out_bad_at, S.bad_at.data(), N * 4);
  memcpy(out_writers, S.writers.data(), S.n_writers * 8);
  *out_n_writers = S.n_writers;
  if (out_stats) { out_stats[0] = S.ms; out_stats[1] = (float)S.certified_slots; out_stats[2] = ms_chain; out_stats[3] = ms_since(t_call); }
  return CG1_OK;
}
}  // extern "C"
