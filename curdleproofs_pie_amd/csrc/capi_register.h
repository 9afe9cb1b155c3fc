// C ABI, part 20: Whisk registrations made in bulk (kernels_register.h) -- the device call, its host twin on the worker pool and the
// host's copy of the seed derivation.  Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

namespace {
constexpr size_t REG_SLICE = (size_t)1 << 20;             // items per launch chain of the device call: bounds its scratch (1 092 B per item)
// The five multiples of a slice: above this many items k_register_points (one lane and one inversion per ITEM), up to it k_generator_mul
// over the 5 n scalars (one lane and one inversion per POINT).  A lane of k_register_points runs its five sums one after another, ~2 ms
// of dependent additions however few items there are; with five times the lanes k_generator_mul is through in a third of that until the
// lanes fill the chip.  Measured on the stage alone (profiles/r22_registration_timing.txt; the table in DESIGN.md section 22): the
// per-point kernel is 2.4 times faster at 1 024 items, the two cross between 16 384 and 32 768, and the shared inversion is 1.7 times
// faster at 2^20.
constexpr size_t REG_SHARED_MIN_ITEMS = 32768;

// the refusals both twins share, made before anything is written; `err` (nullable) receives the text, which never holds a secret
int register_refuse(char* err, size_t errlen, const char* who, size_t n, const uint8_t* ks32, const uint8_t* rs32, const uint8_t* blinders32, const uint8_t* seed32,
                    bool needs_draws, uint64_t first_index, const uint8_t* out_trackers96, const uint8_t* out_k_commitments48, const uint8_t* out_proofs128,
                    const int32_t* status) {
  const char* why = nullptr;
  if (n >= CG1_WHISK_REGISTER_MAX_ITEMS) why = "more items than one call takes";
  else if (first_index + n > (1ull << 32)) why = "first_index + n passes 2^32";
  else if (!n) return CG1_OK;
  else if (!ks32 || !out_trackers96 || !out_k_commitments48 || !out_proofs128 || !status) why = "a null buffer";
  else if ((rs32 == nullptr) != (blinders32 == nullptr)) why = "rs32 and blinders32 are both given or both NULL";
  else if (!rs32 && (!needs_draws || !seed32)) why = "neither (rs32, blinders32) nor a seed";
  if (!why) return CG1_OK;
  if (err) snprintf(err, errlen, "%s: %s (%zu items)", who, why, n);
  return CG1_ERR_ARG;
}

// draw d (0: r, 1: b) of registration `index`: kernels_register.h draw_from_seed on the host
cg1fr::fr register_draw(const uint8_t seed32[32], uint64_t index, uint32_t d) {
  uint8_t msg[67], st[64];
  memcpy(msg, "whisk_registration_draw", 23);
  memcpy(msg + 23, seed32, 32);
  for (int b = 0; b < 8; ++b) msg[55 + b] = (uint8_t)(index >> (8 * b));
  for (int b = 0; b < 4; ++b) msg[63 + b] = (uint8_t)(d >> (8 * b));
  cg1::shake256_block64(msg, sizeof msg, st);
  const cg1fr::fr v = cg1fr::fr_from_le64_wide(st);
  cg1::wipe(msg, sizeof msg); cg1::wipe(st, sizeof st);
  return v;
}

// The host twin's table of G: unsigned 8-bit windows over affine entries, entry w * 255 + (d - 1) = d * 256^w * G (never the identity:
// d * 256^w is no multiple of the prime r), 32 mixed additions per multiple.  Built at the first call.
struct RegisterGenTable {
  std::vector<cg1h::fe> xs, ys;
  RegisterGenTable() {
    std::vector<cg1h::jac> t(32 * 255);
    cg1h::jac base = cg1h::jac_generator();
    for (int w = 0; w < 32; ++w) {
      cg1h::jac acc = base;
      for (int d = 1; d <= 255; ++d) { t[(size_t)w * 255 + (d - 1)] = acc; acc = cg1h::jac_add(acc, base); }
      base = acc;
    }
    xs.resize(t.size()); ys.resize(t.size());
    std::vector<uint8_t> inf(t.size());
    cg1h::jac_batch_to_affine(t.data(), t.size(), xs.data(), ys.data(), inf.data());
  }
  cg1h::jac mul(const cg1fr::fr& k) const {
    uint8_t le[32];
    cg1fr::fr_to_le32(k, le);
    cg1h::jac acc = cg1h::jac_identity();
    for (int w = 0; w < 32; ++w)
      if (le[w]) { const size_t e = (size_t)w * 255 + (le[w] - 1); acc = cg1h::jac_madd(acc, xs[e], ys[e]); }
    cg1::wipe(le, sizeof le);
    return acc;
  }
};
}  // namespace

extern "C" {
int cg1_whisk_register_draws(const uint8_t seed32[32], uint64_t first_index, size_t n, uint8_t* out_rs32, uint8_t* out_blinders32) {
  if (!seed32 || (n && (!out_rs32 || !out_blinders32)) || first_index + n > (1ull << 32)) return CG1_ERR_ARG;
  for (size_t i = 0; i < n; ++i) {
    cg1fr::fr_to_le32(register_draw(seed32, first_index + i, 0), out_rs32 + 32 * i);
    cg1fr::fr_to_le32(register_draw(seed32, first_index + i, 1), out_blinders32 + 32 * i);
  }
  return CG1_OK;
}

// The host twin: one item at a time on the worker pool, the same bytes and codes as the device call.
int cg1_whisk_register(size_t n, const uint8_t* ks32, const uint8_t* rs32, const uint8_t* blinders32, uint8_t* out_trackers96, uint8_t* out_k_commitments48,
                       uint8_t* out_proofs128, int32_t* status) {
  { const int rc = register_refuse(nullptr, 0, "cg1_whisk_register", n, ks32, rs32, blinders32, nullptr, false, 0, out_trackers96, out_k_commitments48, out_proofs128, status);
    if (rc) return rc; }
  if (n == 0) return CG1_OK;
  using cg1fr::fr;
  static const RegisterGenTable* gtab = new RegisterGenTable;
  uint8_t G48[48];
  cg1h::g1_compress(cg1h::jac_generator(), G48);
  auto one = [&](size_t i) {
    uint8_t *trk = out_trackers96 + 96 * i, *kc = out_k_commitments48 + 48 * i, *pf = out_proofs128 + 128 * i;
    memset(trk, 0, 96); memset(kc, 0, 48); memset(pf, 0, 128);
    fr k, r, b;
    if (!cg1fr::fr_from_le32(ks32 + 32 * i, k)) { status[i] = CG1_SHUFFLE_BAD_SCALAR; return; }
    if (!cg1fr::fr_from_le32(rs32 + 32 * i, r) || cg1fr::fr_is_zero(r) || !cg1fr::fr_from_le32(blinders32 + 32 * i, b) || cg1fr::fr_is_zero(b)) {
      status[i] = CG1_OPENING_BAD_BLINDER;
      return;
    }
    fr sc[5] = {r, cg1fr::fr_mul(k, r), k, b, cg1fr::fr_mul(b, r)};       // r_G, k_r_G, k_G, A, B
    cg1h::jac pts[5];
    for (int j = 0; j < 5; ++j) pts[j] = gtab->mul(sc[j]);
    cg1h::fe xs[5], ys[5];
    uint8_t inf[5], enc[5][48];
    cg1h::jac_batch_to_affine(pts, 5, xs, ys, inf);                       // one inversion per item
    for (int j = 0; j < 5; ++j) cg1h::g1_compress_affine(xs[j], ys[j], inf[j] != 0, enc[j]);
    uint8_t tr[CG1_MERLIN_STATE_BYTES], c32[32];
    cg1_merlin_init(tr, (const uint8_t*)"whisk_opening_proof", 19);
    const uint8_t* order[6] = {enc[2], G48, enc[1], enc[0], enc[3], enc[4]};                   // k_G G k_r_G r_G A B (opening.py:45-48)
    for (const uint8_t* p : order) cg1_merlin_append(tr, (const uint8_t*)"tracker_opening_proof", 21, p, 48);
    cg1_merlin_challenge_scalar(tr, (const uint8_t*)"tracker_opening_proof_challenge", 31, c32);
    fr c;
    cg1fr::fr_from_le32(c32, c);                                          // canonical by construction
    memcpy(trk, enc[0], 48); memcpy(trk + 48, enc[1], 48);
    memcpy(kc, enc[2], 48);
    memcpy(pf, enc[3], 48); memcpy(pf + 48, enc[4], 48);
    cg1fr::fr_to_le32(cg1fr::fr_sub(b, cg1fr::fr_mul(c, k)), pf + 96);    // s = b - c k (opening.py:52)
    status[i] = 0;
    cg1::wipe(sc, sizeof sc); cg1::wipe(&k, sizeof k); cg1::wipe(&r, sizeof r); cg1::wipe(&b, sizeof b);
    cg1::wipe(pts, sizeof pts);
  };
  // slices of 4 items over the worker pool; fewer than 8 items on the caller's thread
  cg1::pool_for((n + 3) / 4, n < 8 ? 1 : 0, [&](size_t it) { for (size_t i = it * 4; i < std::min(n, it * 4 + 4); ++i) one(i); });
  return CG1_OK;
}

// The five multiples of G of n items on the device, the stage the two candidate kernels were measured on (tools/gpu_registration_timing.py):
// d_scalars32 = five columns of n canonical scalars, d_out48 = five columns of n encodings, column for column.  shared_inversion != 0:
// k_register_points (one lane and one inversion per item); 0: k_generator_mul over the 5 n scalars (one lane and one inversion per
// point).  cg1_whisk_register_device takes the first above REG_SHARED_MIN_ITEMS items and the second up to it.  Device pointers; waits
// for the stream.
int cg1_whisk_register_points_device(cg1_ctx* ctx, const void* d_scalars32, size_t n, void* d_out48, int shared_inversion) {
  if (!ctx) return CG1_ERR_HIP;
  if (n == 0) return CG1_OK;
  if (!d_scalars32 || !d_out48 || n > REG_SLICE) return CG1_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  { const int rc = ensure_generator_table(ctx); if (rc) return rc; }
  if (shared_inversion) {
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, cg1reg::REG_MAX_BLOCKS);
    DevBuf park;
    HIPCHK(park.alloc((size_t)blocks * 256 * cg1reg::REG_PARK_WORDS * 4));
    hipLaunchKernelGGL(cg1reg::k_register_points, dim3(blocks), dim3(256), 0, ctx->stream, (const cg1::PreparedPoint*)ctx->d_gen_tab, (const uint32_t*)d_scalars32,
                       (uint32_t)n, (uint32_t*)park.p, (uint32_t*)d_out48);
    HIPCHK(hipStreamSynchronize(ctx->stream));
  } else {
    launch_generator_mul(ctx, d_scalars32, 5 * n, nullptr, d_out48);
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  HIPCHK(hipGetLastError());
  return CG1_OK;
}

// n registrations on the device: host buffers in and out, slices of REG_SLICE items through one launch chain each on the context's stream.
int cg1_whisk_register_device(cg1_ctx* ctx, size_t n, const uint8_t* ks32, const uint8_t* rs32, const uint8_t* blinders32, const uint8_t* seed32,
                              uint64_t first_index, uint8_t* out_trackers96, uint8_t* out_k_commitments48, uint8_t* out_proofs128, int32_t* status) {
  if (!ctx) return CG1_ERR_HIP;
  { const int rc = register_refuse(ctx->err, sizeof ctx->err, "cg1_whisk_register_device", n, ks32, rs32, blinders32, seed32, true, first_index, out_trackers96,
                                   out_k_commitments48, out_proofs128, status);
    if (rc) return rc; }
  if (n == 0) return CG1_OK;
  HIPCHK(hipSetDevice(ctx->device));
  { const int rc = ensure_generator_table(ctx); if (rc) return rc; }
  const size_t cap = std::min(n, REG_SLICE);
  const unsigned max_blocks = cap > REG_SHARED_MIN_ITEMS ? (unsigned)std::min<size_t>((cap + 255) / 256, cg1reg::REG_MAX_BLOCKS) : 0u;   // no parking for a small call
  // scratch per item: k 32 | r 32 | b 32 | scalars 160 | encodings 240 | rows 288 | challenges 32 | status 4 | proofs 128 | k_G 48 | trackers 96;
  // then k_register_points' parking, 1 120 B per lane of its grid
  const size_t per = 32 + 32 + 32 + 160 + 240 + cg1open::ROW_BYTES + 32 + 4 + 128 + 48 + 96, o_park = (per * cap + 255) & ~(size_t)255,
               need = o_park + (size_t)max_blocks * 256 * cg1reg::REG_PARK_WORDS * 4;
  if (const int rc = cg1::grow_bufs(ctx, ctx->cap_register, need, need, {cg1::dev_buf(ctx->d_register, need)})) return rc;
  hipStream_t st = ctx->stream;
  cg1open::Seed32 seed{};
  if (!rs32) memcpy(seed.w, seed32, 32);
  uint8_t gblob[CG1_POINT_BYTES], g48[48];
  cg1_generator(gblob);
  cg1_compress(g48, gblob);
  cg1open::Enc48 genc;
  memcpy(genc.w, g48, 48);
  uint8_t init[CG1_MERLIN_STATE_BYTES];
  cg1_merlin_op ops[7];
  opening_transcript_program(init, ops);
  int rc = CG1_OK;
  for (size_t lo = 0; lo < n && rc == CG1_OK; lo += REG_SLICE) {
    const size_t m = std::min(REG_SLICE, n - lo);
    const uint32_t m32 = (uint32_t)m;
    uint8_t* base = (uint8_t*)ctx->d_register;
    uint8_t *d_k = base, *d_r = d_k + 32 * m, *d_b = d_r + 32 * m, *d_sc = d_b + 32 * m, *d_enc = d_sc + 160 * m, *d_rows = d_enc + 240 * m,
            *d_ch = d_rows + (size_t)cg1open::ROW_BYTES * m, *d_st = d_ch + 32 * m, *d_pf = d_st + 4 * m, *d_kc = d_pf + 128 * m, *d_trk = d_kc + 48 * m;
    uint8_t *d_gen48 = d_enc, *d_wire = d_enc + 96 * m, *d_b48 = d_enc + 192 * m;          // [k_G | A], [r_G | k_r_G], [B]: the opening prover's three buffers
    // every exit below this point passes the wipe of the secret columns: k, r, b and the five scalars
    auto chain = [&]() -> int {
      HIPCHK(hipMemcpyAsync(d_k, ks32 + 32 * lo, 32 * m, hipMemcpyHostToDevice, st));
      if (rs32) {
        HIPCHK(hipMemcpyAsync(d_r, rs32 + 32 * lo, 32 * m, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_b, blinders32 + 32 * lo, 32 * m, hipMemcpyHostToDevice, st));
      }
      hipLaunchKernelGGL(cg1reg::k_register_scalars, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, (const uint8_t*)d_k, rs32 ? (const uint8_t*)d_r : (const uint8_t*)nullptr,
                         rs32 ? (const uint8_t*)d_b : (const uint8_t*)nullptr, seed, (uint32_t)(first_index + lo), m32, (int32_t)CG1_SHUFFLE_BAD_SCALAR,
                         (int32_t)CG1_OPENING_BAD_BLINDER, d_sc, (int32_t*)d_st);
      if (m > REG_SHARED_MIN_ITEMS) {
        const unsigned blocks = (unsigned)std::min<size_t>((m + 255) / 256, max_blocks);
        hipLaunchKernelGGL(cg1reg::k_register_points, dim3(blocks), dim3(256), 0, st, (const cg1::PreparedPoint*)ctx->d_gen_tab, (const uint32_t*)d_sc, m32,
                           (uint32_t*)(base + o_park), (uint32_t*)d_enc);
      } else {
        launch_generator_mul(ctx, d_sc, 5 * m, nullptr, d_enc);                                // the same columns, one inversion per point
      }
      hipLaunchKernelGGL(cg1open::k_prove_gather, dim3((unsigned)((6 * m + 255) / 256)), dim3(256), 0, st, (const uint32_t*)d_gen48, (const uint32_t*)d_b48,
                         (const uint32_t*)d_wire, genc, m32, (uint32_t*)d_rows);
      if (const int r2 = cg1_merlin_batch_device(ctx, init, ops, 7, d_rows, cg1open::ROW_BYTES, d_ch, 32, nullptr, m)) return r2;
      hipLaunchKernelGGL(cg1open::k_prove_response, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (const uint8_t*)d_ch, (const uint8_t*)d_sc,
                         (const uint32_t*)d_gen48, (const uint32_t*)d_b48, (const int32_t*)d_st, m32, (uint32_t*)d_pf, (uint32_t*)d_kc);
      hipLaunchKernelGGL(cg1reg::k_register_trackers, dim3((unsigned)((2 * m + 255) / 256)), dim3(256), 0, st, (const uint32_t*)d_wire, (const int32_t*)d_st, m32,
                         (uint32_t*)d_trk);
      HIPCHK(hipMemcpyAsync(out_trackers96 + 96 * lo, d_trk, 96 * m, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(out_k_commitments48 + 48 * lo, d_kc, 48 * m, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(out_proofs128 + 128 * lo, d_pf, 128 * m, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(status + lo, d_st, 4 * m, hipMemcpyDeviceToHost, st));
      return CG1_OK;
    };
    rc = chain();
    const hipError_t ew = hipMemsetAsync(d_k, 0, (32 + 32 + 32 + 160) * m, st);             // k | r | b | scalars are contiguous
    const hipError_t es = hipStreamSynchronize(st);
    if (rc == CG1_OK) { HIPCHK(ew); HIPCHK(es); HIPCHK(hipGetLastError()); }
  }
  return rc;
}
}  // extern "C"
