// C ABI, part 19: the tracker scan -- which trackers a set of secrets opens (kernels_tracker_scan.h) -- on the device and its host twin.
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

namespace {
static_assert(CG1_TRACKER_MATCH_MAX_TILE <= 65535, "a tile's trackers are the y dimension of k_tracker_match's grid");
static_assert(CG1_TRACKER_MATCH_DEFAULT_TILE <= CG1_TRACKER_MATCH_MAX_TILE, "");

// the refusals both twins share, made before anything is written; `err` (nullable) receives the text, which never holds a secret
int tracker_match_refuse(char* err, size_t errlen, const char* who, const uint8_t* trackers96, size_t T, const uint8_t* ks32, size_t V, size_t tile,
                         const uint64_t* out_bitmap, const int32_t* out_tracker_status, const int32_t* out_k_status) {
  const char* why = nullptr;
  if (T > CG1_TRACKER_MATCH_MAX_TRACKERS || V > CG1_TRACKER_MATCH_MAX_KS) why = "more trackers or secrets than one call takes";
  else if (tile > CG1_TRACKER_MATCH_MAX_TILE) why = "tile_bases above CG1_TRACKER_MATCH_MAX_TILE";
  else if ((uint64_t)T * ((V + 63) / 64) * 8ull > CG1_TRACKER_MATCH_MAX_BITMAP_BYTES) why = "the bitmap exceeds CG1_TRACKER_MATCH_MAX_BITMAP_BYTES";
  else if ((T && (!trackers96 || !out_tracker_status)) || (V && (!ks32 || !out_k_status)) || (T && V && !out_bitmap)) why = "a null buffer";
  if (!why) return CG1_OK;
  if (err) snprintf(err, errlen, "%s: %s (%zu trackers, %zu secrets)", who, why, T, V);
  return CG1_ERR_ARG;
}

void tracker_match_k_status(const uint8_t* ks32, size_t V, int32_t* out_k_status) {
  for (size_t j = 0; j < V; ++j) {
    uint32_t s[8];
    memcpy(s, ks32 + 32 * j, 32);
    out_k_status[j] = cg1::fixed_scalar_below_r(s) ? 0 : CG1_SHUFFLE_BAD_SCALAR;
  }
}
}  // namespace

extern "C" {
int cg1_tracker_match_device(cg1_ctx* ctx, const uint8_t* trackers96, size_t n_trackers, const uint8_t* ks32, size_t n_ks, size_t tile_bases,
                             uint64_t* out_bitmap, int32_t* out_tracker_status, int32_t* out_k_status) {
  if (!ctx) return CG1_ERR_HIP;
  const size_t T = n_trackers, V = n_ks;
  { const int rc = tracker_match_refuse(ctx->err, sizeof ctx->err, "cg1_tracker_match_device", trackers96, T, ks32, V, tile_bases, out_bitmap, out_tracker_status, out_k_status);
    if (rc) return rc; }
  ctx->tscan_ms[0] = ctx->tscan_ms[1] = 0.f;
  if (V) tracker_match_k_status(ks32, V, out_k_status);
  if (T == 0) return CG1_OK;
  const size_t tile = tile_bases ? tile_bases : (size_t)CG1_TRACKER_MATCH_DEFAULT_TILE, words = (V + 63) / 64;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // the tile's table lives with the context (records of public points); the secrets get a buffer of their own that is wiped and freed
  // a handful of secrets: one ladder per pair instead of a table per tracker (kernels_tracker_scan.h; "tracker_scan_ladder_max_ks")
  const bool ladder = V && V <= (size_t)ctx->tscan_ladder_max_ks && T * V <= ((size_t)1 << 24);
  const size_t tab_bytes = std::min(tile, T) * (size_t)cg1::LT_ENTRIES * sizeof(cg1::PointSum);
  if (V && !ladder) { const int rc = cg1::grow_bufs(ctx, ctx->cap_tscan_tab, tab_bytes, tab_bytes, {cg1::dev_buf(ctx->d_tscan_tab, tab_bytes)}); if (rc) return rc; }
  // scratch: trackers 96 | wire 96 | affine 192 | point status 2 (padded) | bitmap 8 words, per tracker; the ladder route: V products 96
  const size_t o_wire = 96 * T, o_aff = o_wire + 96 * T, o_ps = o_aff + 192 * T, o_bm = (o_ps + 2 * T + 15) & ~(size_t)15,
               o_prod = (o_bm + 8 * words * T + 15) & ~(size_t)15, bytes = o_prod + (ladder ? 96 * T * V : 0);
  const size_t sec_bytes = 32 * V + (ladder ? 32 * T * V : 0);
  DevBuf pub, sec;
  HIPCHK(pub.alloc(bytes));
  uint8_t* D = (uint8_t*)pub.p;
  HIPCHK(hipMemcpyAsync(D, trackers96, 96 * T, hipMemcpyHostToDevice, st));
  if (V) {
    HIPCHK(sec.alloc(sec_bytes));
    HIPCHK(hipMemcpyAsync(sec.p, ks32, 32 * V, hipMemcpyHostToDevice, st));
  }
  hipLaunchKernelGGL(cg1open::k_prove_split, dim3((unsigned)((2 * T + 255) / 256)), dim3(256), 0, st, (const uint32_t*)D, (uint32_t)T, (uint32_t*)(D + o_wire));
  launch_decompress(ctx, D + o_wire, D + o_aff, D + o_ps, 2 * T, 0);       // [r_G ...][k_r_G ...], unchecked (util.py:35-36)
  const bool timed = ctx->tscan_timing != 0;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<float, std::milli>(b - a).count(); };
  if (ladder) {
    std::chrono::steady_clock::time_point c0;
    if (timed) { HIPCHK(hipStreamSynchronize(st)); c0 = now(); }
    const uint32_t n = (uint32_t)(T * V);
    uint32_t* d_rep = (uint32_t*)sec.p + 8 * V;
    hipLaunchKernelGGL(cg1::k_tracker_replicate, dim3((n + 255) / 256), dim3(256), 0, st, (const uint32_t*)sec.p, (uint32_t)V, (uint32_t)T, d_rep);
    hipLaunchKernelGGL(cg1::k_batch_mul, dim3((n + 127) / 128), dim3(128), 0, st, (const uint32_t*)(D + o_aff), (uint32_t)T, (const uint32_t*)d_rep, n,
                       (const uint32_t*)nullptr, (uint32_t*)(D + o_prod), n);
    hipLaunchKernelGGL(cg1::k_tracker_compare, dim3((unsigned)((T * words + 255) / 256)), dim3(256), 0, st, (const uint32_t*)(D + o_prod),
                       (const uint32_t*)(D + o_aff + 96 * T), (const uint8_t*)(D + o_ps), (const uint8_t*)(D + o_ps + T), (const uint32_t*)sec.p, (uint32_t)V,
                       (uint32_t)T, (unsigned long long*)(D + o_bm), (uint32_t)words);
    if (timed) { HIPCHK(hipStreamSynchronize(st)); ctx->tscan_ms[1] += ms(c0, now()); }
  }
  for (size_t t0 = 0; V && !ladder && t0 < T; t0 += tile) {
    const size_t nt = std::min(tile, T - t0), nrec = nt * (size_t)cg1::LT_ENTRIES;
    cg1::PointSum* tab = (cg1::PointSum*)ctx->d_tscan_tab;
    std::chrono::steady_clock::time_point c0, c1;
    if (timed) { HIPCHK(hipStreamSynchronize(st)); c0 = now(); }
    light_build(ctx, D + o_aff + 96 * t0, nt, tab);
    hipLaunchKernelGGL(cg1::k_tracker_normalise, dim3((unsigned)((nrec * 4 + 255) / 256)), dim3(256), 0, st, tab, (uint32_t)nrec);
    if (timed) { HIPCHK(hipStreamSynchronize(st)); c1 = now(); ctx->tscan_ms[0] += ms(c0, c1); }
    hipLaunchKernelGGL(cg1::k_tracker_match, dim3((unsigned)words, (unsigned)nt), dim3(64), 0, st, (const cg1::PointSum*)tab,
                       (const uint32_t*)(D + o_aff + 96 * (T + t0)), (const uint8_t*)(D + o_ps + t0), (const uint8_t*)(D + o_ps + T + t0), (const uint32_t*)sec.p,
                       (uint32_t)V, (uint32_t)nt, (unsigned long long*)(D + o_bm) + t0 * words, (uint32_t)words);
    if (timed) { HIPCHK(hipStreamSynchronize(st)); ctx->tscan_ms[1] += ms(c1, now()); }
  }
  std::vector<uint8_t> ps(2 * T);
  HIPCHK(hipMemcpyAsync(ps.data(), D + o_ps, 2 * T, hipMemcpyDeviceToHost, st));
  if (V) {
    HIPCHK(hipMemcpyAsync(out_bitmap, D + o_bm, 8 * words * T, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemsetAsync(sec.p, 0, sec_bytes, st));                         // the secrets do not outlive the call on the device
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  for (size_t i = 0; i < T; ++i) out_tracker_status[i] = (ps[i] | ps[T + i]) ? CG1_SHUFFLE_BAD_POINT : 0;
  return CG1_OK;
}

int cg1_tracker_match_last_ms(const cg1_ctx* ctx, float ms[2]) {
  if (!ctx || !ms) return CG1_ERR_ARG;
  ms[0] = ctx->tscan_ms[0]; ms[1] = ctx->tscan_ms[1];
  return CG1_OK;
}

// The host twin: decode, multiply, compare (host_g1.cpp), items of one tracker x 64 secrets -- one word of the bitmap -- over the worker pool.
int cg1_tracker_match(const uint8_t* trackers96, size_t n_trackers, const uint8_t* ks32, size_t n_ks, size_t tile_bases, uint64_t* out_bitmap,
                      int32_t* out_tracker_status, int32_t* out_k_status) {
  const size_t T = n_trackers, V = n_ks, words = (V + 63) / 64;
  { const int rc = tracker_match_refuse(nullptr, 0, "cg1_tracker_match", trackers96, T, ks32, V, tile_bases, out_bitmap, out_tracker_status, out_k_status);
    if (rc) return rc; }
  if (V) tracker_match_k_status(ks32, V, out_k_status);
  if (T == 0) return CG1_OK;
  using cg1h::jac;
  std::vector<jac> Rs(T), Ss(T);
  auto decode = [&](size_t i) {
    const bool bad = cg1h::g1_decompress(trackers96 + 96 * i, false, Rs[i]) != 0 || cg1h::g1_decompress(trackers96 + 96 * i + 48, false, Ss[i]) != 0;
    out_tracker_status[i] = bad ? CG1_SHUFFLE_BAD_POINT : 0;
  };
  auto word = [&](size_t it) {
    const size_t i = it / words, wj = it % words;
    uint64_t bits = 0;
    if (out_tracker_status[i] == 0)
      for (size_t j = 64 * wj; j < std::min(V, 64 * wj + 64); ++j)
        if (out_k_status[j] == 0 && cg1h::jac_eq(cg1h::jac_mul(Rs[i], ks32 + 32 * j), Ss[i])) bits |= 1ull << (j & 63);
    out_bitmap[it] = bits;
  };
  cg1::pool_for(T, T < 16 ? 1 : 0, decode);                 // (fewer than 16 decodings do not pay for waking the pool)
  cg1::pool_for(T * words, 0, word);
  return CG1_OK;
}
}  // extern "C"
