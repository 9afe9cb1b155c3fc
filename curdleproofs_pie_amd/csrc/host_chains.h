// Host side of the MSM engine, part 3: the launch chains (regime A, the single-launch small MSM, regime B) as stages over a plan (msm_plan.h).
// Part of the single translation unit csrc/msm_gpu.hip (included there, in this order; not a stand-alone header).
#pragma once

namespace cg1 {

// Wait for the context's compute stream.  blocking_sync: sleep until the GPU signals (an event created with
// hipEventBlockingSync) and leave the core to the front-end threads; default: the runtime's spinning wait (lowest latency).
static int wait_stream(Ctx* ctx) {
  if (ctx->blocking_sync) {
    HIPCHK(hipEventRecord(ctx->sync_ev, ctx->stream));
    HIPCHK(hipEventSynchronize(ctx->sync_ev));
    return CG1_OK;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return CG1_OK;
}

// Wait, spinning, for the sequence number a call's last kernel stores into the context's flag word (mapped host memory) once everything
// it exports is there; look at the stream now and then so that a failed launch cannot hang us.
static int wait_export_flag(Ctx* ctx, uint32_t seq) {
  volatile uint32_t* flag = ctx->h_flag;
  for (uint32_t spins = 0; *flag != seq; ++spins) {
    if ((spins & 0x3fffu) == 0x3fffu) {
      hipError_t q = hipStreamQuery(ctx->stream);
      if (q == hipSuccess) { if (*flag != seq) { snprintf(ctx->err, sizeof ctx->err, "the stream drained without the export flag"); return CG1_ERR_HIP; } break; }
      if (q != hipErrorNotReady) { snprintf(ctx->err, sizeof ctx->err, "stream failed: %s", hipGetErrorString(q)); return CG1_ERR_HIP; }
    }
    __builtin_ia32_pause();
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return CG1_OK;
}

// Where an MSM's points come from (all device memory):
//   AFFINE96  n x 96 B standard-form affine records (the C ABI's "affine96")                      -> k_prepare_points
//   BLOBS     n x 144 B host point blobs as G1Point objects hold them (Jacobian, radix 2^384)     -> k_prepare_blobs
//   PREPARED  n x 128 B records + n identity flags made earlier by one of the two (a cg1_vec)    -> nothing to do
struct PtSrc {
  enum Kind { AFFINE96 = 0, BLOBS = 1, PREPARED = 2 } kind = AFFINE96;
  const void* p = nullptr;
  const uint8_t* flags = nullptr;       // PREPARED only
  bool normalised = false;              // BLOBS only: every Z is 0 or 1 (no inversion needed)
  PtSrc() {}
  PtSrc(const void* affine96) : p(affine96) {}
};

// points per lane of k_prepare_blobs<true>: one Fermat inversion per lane, so few lanes for big inputs -- but never fewer than
// ~2 waves per SIMD's worth, where the launch turns from latency- into throughput-bound
static uint32_t blob_points_per_lane(size_t n) {
  size_t K = (n + (1u << 17) - 1) >> 17;
  return (uint32_t)(K < 1 ? 1 : (K > 16 ? 16 : K));
}

// records + flags from `src` into (out, flags_out) on `st`; clears the call's status words (like k_prepare_points)
static void launch_prepare(hipStream_t st, const PtSrc& src, PreparedPoint* out, uint8_t* flags_out, uint32_t n32, uint32_t* status_words) {
  if (src.kind == PtSrc::AFFINE96) {
    hipLaunchKernelGGL(k_prepare_points, dim3((n32 + 255) / 256), dim3(256), 0, st, (const uint32_t*)src.p, out, flags_out, n32, status_words);
  } else if (src.normalised) {
    hipLaunchKernelGGL((k_prepare_blobs<false>), dim3((n32 + 127) / 128), dim3(128), 0, st, (const uint32_t*)src.p, out, flags_out, n32, 1u, status_words);
  } else {
    const uint32_t K = blob_points_per_lane(n32);
    const uint32_t lanes = (n32 + K - 1) / K;
    hipLaunchKernelGGL((k_prepare_blobs<true>), dim3((lanes + 127) / 128), dim3(128), 0, st, (const uint32_t*)src.p, out, flags_out, n32, K, status_words);
  }
}

// Enqueue the whole launch chain of this context's share of an MSM (windows w = rank mod world of the plan) up to the D2H of
// the window sums; nothing waits.
// Hooks of the two-chain form of one call (msm_begin_split): `after_prepare` is recorded on the chain's stream once the prepared
// records exist (the other chain reads them); the chain waits for `before_start` before its first launch and for
// `before_accumulate` in front of k_accumulate; `after_accumulate` is recorded behind k_accumulate.
struct ChainHooks {
  hipEvent_t before_start = nullptr, after_prepare = nullptr, before_accumulate = nullptr, after_accumulate = nullptr;
};

// ---- the stages of a launch chain: each enqueues what the plan says on the context's stream, nothing waits
// bucket offsets and chunk offsets from the bucket histogram (both sorts, both regimes)
static void stage_scan3(Ctx* ctx, size_t nb_total, uint32_t L) {
  const uint32_t nblk = (uint32_t)((nb_total + SCAN_ITEMS - 1) / SCAN_ITEMS);
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_scan1, dim3(nblk), dim3(256), 0, st, ctx->d_hist, ctx->d_off, ctx->d_choff, ctx->d_blocktot, (uint32_t)nb_total, L);
  hipLaunchKernelGGL(k_scan2, dim3(1), dim3(256), 0, st, ctx->d_blocktot, nblk, ctx->d_off, ctx->d_choff, (uint32_t)nb_total);
  hipLaunchKernelGGL(k_scan3, dim3(nblk), dim3(256), 0, st, ctx->d_blocktot, ctx->d_off, ctx->d_choff, (uint32_t)nb_total);
}

// front: the prepared records (unless they exist) and the cleared status words
static int stage_front(Ctx* ctx, const ChainPlan& cp, const PtSrc& src, const ChainHooks& hooks, uint32_t* bad_flag) {
  hipStream_t st = ctx->stream;
  const uint32_t n_real32 = (uint32_t)cp.n_real;
  if (hooks.before_start) HIPCHK(hipStreamWaitEvent(st, hooks.before_start, 0));
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[0], st));
  if (cp.resident) HIPCHK(hipMemsetAsync(bad_flag, 0, 16, st));                    // (an endomorphism-split call: the source already holds both halves)
  else {
    launch_prepare(st, src, ctx->d_pts, ctx->d_flags, n_real32, bad_flag);
    if (cp.plan.glv) hipLaunchKernelGGL(k_phi_records, dim3((n_real32 + 255) / 256), dim3(256), 0, st, ctx->d_pts, ctx->d_flags, n_real32);
  }
  if (hooks.after_prepare) HIPCHK(hipEventRecord(hooks.after_prepare, st));
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[1], st));
  return CG1_OK;
}

// sort, two-level partition form: digits, partition counts and their scan, scatter into bins, one workgroup per bin (giant bins by slices), bucket scan
static int stage_partition_sort(Ctx* ctx, const ChainPlan& cp, const void* d_scalars32, const uint8_t* flags, uint32_t* bad_flag) {
  hipStream_t st = ctx->stream;
  const uint32_t n32 = (uint32_t)cp.n, n_real32 = (uint32_t)cp.n_real, nlw = (uint32_t)cp.nlw, nslices = cp.nslices, nbins = cp.nbins, sub_bits = cp.sub_bits, nbc = cp.nbc;
  hipLaunchKernelGGL(k_digits, dim3((n_real32 + 255) / 256), dim3(256), 0, st, (const uint32_t*)d_scalars32, flags, ctx->d_digits, n_real32, cp.plan, cp.rank, cp.world, bad_flag);
  hipLaunchKernelGGL(k_part_count, dim3(nslices, nlw), dim3(256), 0, st, ctx->d_digits, ctx->d_blockcnt, n32, nslices, nbins, sub_bits);
  const uint32_t ublk = (nbc + SCAN_ITEMS - 1) / SCAN_ITEMS;
  if (cp.uscan_one) {
    hipLaunchKernelGGL(k_uscan_one, dim3(1), dim3(1024), 0, st, ctx->d_blockcnt, nbc);
  } else {
    hipLaunchKernelGGL(k_uscan1, dim3(ublk), dim3(256), 0, st, ctx->d_blockcnt, ctx->d_ublocktot, nbc);
    hipLaunchKernelGGL(k_uscan2, dim3(1), dim3(256), 0, st, ctx->d_ublocktot, ublk, ctx->d_blockcnt, nbc);
    hipLaunchKernelGGL(k_uscan3, dim3(ublk), dim3(256), 0, st, ctx->d_ublocktot, ctx->d_blockcnt, nbc);
  }
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[2], st));
  hipLaunchKernelGGL(k_part_scatter, dim3(nslices, nlw), dim3(256), 0, st, ctx->d_digits, ctx->d_blockcnt, ctx->d_part, n32, nslices, nbins, sub_bits, ctx->stage_sort);
  const uint32_t nbt = nlw * nbins;
  hipLaunchKernelGGL(k_slice_plan, dim3(1), dim3(256), 0, st, ctx->d_blockcnt, nbt, nslices, ctx->d_slice_base, ctx->d_bigflag, cp.big_bins);
  hipLaunchKernelGGL(k_bin_sort, dim3(nbt), dim3(256), 0, st, ctx->d_part, ctx->d_blockcnt, ctx->d_hist, ctx->d_sorted, nbt, nslices, sub_bits, ctx->stage_sort, ctx->d_bigflag);
  if (cp.big_bins) {
    const uint32_t max_slices = (uint32_t)((cp.n * (size_t)cp.nlw) / SLICE + nbt + 1);
    hipLaunchKernelGGL(k_slice_count, dim3(max_slices), dim3(256), 0, st, ctx->d_part, ctx->d_blockcnt, nbt, nslices, ctx->d_slice_base, ctx->d_slicehist);
    hipLaunchKernelGGL(k_slice_prefix, dim3(nbt), dim3(256), 0, st, ctx->d_blockcnt, nslices, sub_bits, ctx->d_slice_base, ctx->d_bigflag, ctx->d_slicehist, ctx->d_subbase, ctx->d_hist);
    hipLaunchKernelGGL(k_slice_scatter, dim3(max_slices), dim3(256), 0, st, ctx->d_part, ctx->d_blockcnt, nbt, nslices, ctx->d_slice_base, ctx->d_slicehist, ctx->d_subbase, ctx->d_sorted);
  }
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[3], st));
  if (cp.scan_one) hipLaunchKernelGGL(k_scan_one, dim3(1), dim3(1024), 0, st, ctx->d_hist, ctx->d_off, ctx->d_choff, (uint32_t)cp.nb_total, cp.L);
  else stage_scan3(ctx, cp.nb_total, cp.L);
  return CG1_OK;
}

// sort, global-atomic counting form (any n < 2^31)
static int stage_atomic_sort(Ctx* ctx, const ChainPlan& cp, const void* d_scalars32, const uint8_t* flags, uint32_t* bad_flag) {
  hipStream_t st = ctx->stream;
  const uint32_t n32 = (uint32_t)cp.n, gn = (n32 + 255) / 256;
  HIPCHK(hipMemsetAsync(ctx->d_hist, 0, cp.nb_total * 4, st));
  hipLaunchKernelGGL(k_hist, dim3(gn), dim3(256), 0, st, (const uint32_t*)d_scalars32, flags, ctx->d_hist, n32, cp.plan, cp.rank, cp.world, bad_flag);
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[2], st));
  stage_scan3(ctx, cp.nb_total, cp.L);
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[3], st));
  hipLaunchKernelGGL(k_scatter, dim3(gn), dim3(256), 0, st, (const uint32_t*)d_scalars32, flags, ctx->d_hist, ctx->d_off, ctx->d_sorted, n32, cp.plan, cp.rank, cp.world);
  return CG1_OK;
}

// chunks and accumulate (both regimes): the sorted entries of nb_total buckets cut into chunks of <= L, ordered by length, summed by
// k_accumulate; buckets of many chunks re-joined.  The events of a two-chain form go around k_accumulate.
static int stage_accumulate(Ctx* ctx, size_t nb_total, size_t entries, uint32_t L, const PreparedPoint* pts, uint32_t* bad_flag,
                            hipEvent_t wait_before_accumulate, hipEvent_t record_after_accumulate) {
  hipStream_t st = ctx->stream;
  // one memset: chunk-length histogram, the any_multi flag, combined[] and the heavy-bucket count (ensure() laid them out together)
  HIPCHK(hipMemsetAsync(ctx->d_zblock, 0, zblock_clear_bytes(ctx), st));
  hipLaunchKernelGGL(k_chunk_desc, dim3((uint32_t)std::min<size_t>(CHUNK_DESC_BLOCKS, (nb_total + 255) / 256)), dim3(256), 0, st, ctx->d_off, ctx->d_choff, ctx->d_desc, ctx->d_lenhist, ctx->d_heavy, (uint32_t)ctx->cap_heavy, (uint32_t)nb_total, L, ctx->d_any_multi);
  const size_t max_chunks = nb_total + entries / L + 1;
  const uint32_t gchunks = (uint32_t)((max_chunks + 255) / 256);
  hipLaunchKernelGGL(k_len_scan, dim3(1), dim3(256), 0, st, ctx->d_lenhist, ctx->d_lenhist + LEN_BINS, ctx->d_off + nb_total, ctx->d_choff + nb_total, bad_flag);
  hipLaunchKernelGGL(k_order, dim3((gchunks + ORDER_PER - 1) / ORDER_PER), dim3(256), 0, st, ctx->d_desc, ctx->d_choff + nb_total, ctx->d_lenhist + LEN_BINS, ctx->d_order);
  if (wait_before_accumulate) HIPCHK(hipStreamWaitEvent(st, wait_before_accumulate, 0));
  if (ctx->profile >= 1) HIPCHK(hipEventRecord(ctx->ev[4], st));
  hipLaunchKernelGGL(k_accumulate, dim3(gchunks), dim3(256), 0, st, ctx->d_desc, ctx->d_choff + nb_total, ctx->d_order, ctx->d_sorted, pts, ctx->d_sums);
  if (ctx->profile >= 1) HIPCHK(hipEventRecord(ctx->ev[5], st));
  if (record_after_accumulate) HIPCHK(hipEventRecord(record_after_accumulate, st));
  hipLaunchKernelGGL(k_heavy_combine, dim3(512), dim3(256), 0, st, ctx->d_heavy, (uint32_t)ctx->cap_heavy, ctx->d_choff, ctx->d_sums, ctx->d_combined);
  return CG1_OK;
}

// regime A's tail: fold, then row / column sums and the tree of 1 + hb + lb items per window -- or the 1-D form, segments and bit trees
static int stage_tail(Ctx* ctx, const ChainPlan& cp, uint32_t* bad_flag) {
  hipStream_t st = ctx->stream;
  const TailPlan& t = cp.tail;
  const uint32_t nlw = (uint32_t)cp.nlw, hb2 = cp.hb2, lb2 = cp.lb2, nb32 = (uint32_t)cp.nb_total;
  if (t.fold == FOLD_QUAD) hipLaunchKernelGGL(k_bucket_fold_quad, dim3((uint32_t)((cp.nb_total * 4 + 255) / 256)), dim3(256), 0, st, ctx->d_choff, ctx->d_sums, ctx->d_combined, nb32, ctx->d_any_multi);
  else if (t.fold == FOLD_LANES) hipLaunchKernelGGL(k_bucket_fold, dim3((uint32_t)((cp.nb_total + 255) / 256)), dim3(256), 0, st, ctx->d_choff, ctx->d_sums, ctx->d_combined, nb32, ctx->d_any_multi);
  if (t.rowcol == ROWCOL_SEG) {
    const uint32_t nseg_total = (uint32_t)(cp.nb_total / cp.m);
    hipLaunchKernelGGL(k_seg_reduce, dim3((nseg_total + 255) / 256), dim3(256), 0, st, ctx->d_choff, ctx->d_sums, ctx->d_combined, ctx->d_segrun, ctx->d_segtot, nseg_total, cp.m);
    if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[6], st));
    uint32_t S = (cp.J + BT_ELEMS - 1) / BT_ELEMS; if (S < 1) S = 1; if (S > 64) S = 64;   // J <= 2^15 / seg_m
    hipLaunchKernelGGL(k_bit_tree, dim3(cp.nitems, nlw, S), dim3(256), 0, st, ctx->d_segrun, ctx->d_segtot, ctx->d_partial, cp.J);
    hipLaunchKernelGGL(k_bit_tree_final, dim3((uint32_t)(cp.nitems * nlw)), dim3(64), 0, st, ctx->d_partial, ctx->d_out, S);
    return CG1_OK;
  }
  const uint32_t R = 1u << hb2, Cn = 1u << lb2;
  PointSum* rowsum = ctx->d_segrun;                     // reuse the segment buffers (>= nb_total records each)
  PointSum* colsum = ctx->d_segtot;
  if (t.rowcol == ROWCOL_QUAD_ROW) {
    hipLaunchKernelGGL(k_rowcol_quad_row, dim3((nlw * (R + Cn) + 3u) / 4u), dim3(256), 0, st, ctx->d_choff, ctx->d_sums, ctx->d_combined, rowsum, colsum, nlw, hb2, lb2);
  } else if (t.rowcol == ROWCOL_QUAD) {
    const uint32_t rc_waves = (nlw * (R + Cn) + (16u >> t.lgq) - 1u) / (16u >> t.lgq);
    hipLaunchKernelGGL(k_rowcol_quad, dim3((rc_waves + 3u) / 4u), dim3(256), 0, st, ctx->d_choff, ctx->d_sums, rowsum, colsum, nlw, hb2, lb2, t.lgq);
  } else {
    const uint32_t lpr = Cn < 32u ? Cn : 32u, lpc = R < 16u ? R : 16u;
    const uint32_t nrow_blocks = (nlw * R + (256u / lpr) - 1u) / (256u / lpr);
    const uint32_t ncol_blocks = (nlw * Cn + (256u / lpc) - 1u) / (256u / lpc);
    hipLaunchKernelGGL(k_rowcol, dim3(nrow_blocks + ncol_blocks), dim3(256), 0, st, ctx->d_choff, ctx->d_sums, ctx->d_combined, rowsum, colsum, nlw, hb2, lb2, nrow_blocks, ctx->quad);
  }
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[6], st));
  const dim3 grid(cp.nitems, nlw), block(t.tree_block);
  if (t.tree == TREE_ROW) {
    const bool exports = t.exp == EXPORT_TREE;
    if (exports) ++ctx->seq;
    hipLaunchKernelGGL(k_small_tree_row, grid, block, 0, st, rowsum, colsum, ctx->d_out, hb2, lb2, exports ? ctx->h_out_dev : (PointWords*)nullptr, bad_flag, ctx->h_flag_dev, ctx->seq);
  }
  else if (t.tree == TREE_QUAD) hipLaunchKernelGGL(k_small_tree_quad, grid, block, 0, st, rowsum, colsum, ctx->d_out, hb2, lb2);
  else hipLaunchKernelGGL(k_small_tree, grid, block, 0, st, rowsum, colsum, ctx->d_out, hb2, lb2);
  return CG1_OK;
}

// export: the window sums + status words to the host, unless k_small_tree_row has written the records, the status words and the flag
static int stage_export(Ctx* ctx, const ChainPlan& cp) {
  const size_t bytes = ((size_t)cp.nlw * cp.nitems + 1) * sizeof(PointWords);
  if (cp.tail.exp == EXPORT_KERNEL) {
    // the window sums + status words go straight into mapped host memory, then the call's sequence number into the flag word the
    // host polls: no DMA copy to set up, no stream wait to wake from (~25 us per call, all of it on the critical path of a small MSM)
    ++ctx->seq;
    hipLaunchKernelGGL(k_export_host, dim3(1), dim3(1024), 0, ctx->stream, reinterpret_cast<const uint4*>(ctx->d_out), reinterpret_cast<uint4*>(ctx->h_out_dev), (uint32_t)(bytes / 16),
                       ctx->h_flag_dev, ctx->seq);
  } else if (cp.tail.exp == EXPORT_COPY) {
    HIPCHK(hipMemcpyAsync(ctx->h_out, ctx->d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[7], ctx->stream));
  return CG1_OK;
}

static int msm_enqueue(Ctx* ctx, const PtSrc& src, const void* d_scalars32, size_t n, const WinPlan& plan, int rank, int world,
                       const ChainHooks& hooks = ChainHooks()) {
  ctx->pend.active = false;
  ctx->last_tail = 0;
  HIPCHK(hipSetDevice(ctx->device));
  const ChainPlan cp = plan_regime_a(*ctx, n, plan, rank, world, src.kind == PtSrc::PREPARED);
  if (cp.nlw <= 0) return CG1_OK;
  int rc = ensure(ctx, cp.n, cp.nb_total, cp.nlw, cp.nitems, cp.L, !cp.resident);
  if (rc) return rc;
  auto h0 = std::chrono::steady_clock::now();
  const PreparedPoint* pts = cp.resident ? static_cast<const PreparedPoint*>(src.p) : ctx->d_pts;
  const uint8_t* flags = cp.resident ? src.flags : ctx->d_flags;
  const size_t nout_words = (size_t)cp.nlw * cp.nitems;
  uint32_t* bad_flag = reinterpret_cast<uint32_t*>(ctx->d_out + nout_words);       // [0] set by the digit kernels: a scalar >= 2^255; [1], [2]: counts
  const int profile = ctx->profile;
  if ((rc = stage_front(ctx, cp, src, hooks, bad_flag))) return rc;
  if ((rc = (cp.partition ? stage_partition_sort : stage_atomic_sort)(ctx, cp, d_scalars32, flags, bad_flag))) return rc;
  if ((rc = stage_accumulate(ctx, cp.nb_total, cp.n * (size_t)cp.nlw, cp.L, pts, bad_flag, hooks.before_accumulate, hooks.after_accumulate))) return rc;
  if ((rc = stage_tail(ctx, cp, bad_flag))) return rc;
  if ((rc = stage_export(ctx, cp))) return rc;
  ctx->last_tail = tail_word(cp.tail);
  auto h1 = std::chrono::steady_clock::now();
  Ctx::Pending& pd = ctx->pend;
  pd.zero_copy = ctx->zero_copy != 0; pd.seq = ctx->seq; pd.hout = ctx->h_out;
  pd.active = true; pd.c = plan.cmax; pd.plan = plan; pd.rank = rank; pd.world = world; pd.nlw = cp.nlw; pd.nbits = cp.nbits; pd.m = cp.m; pd.lb2 = cp.lb2; pd.hb2 = cp.hb2;
  pd.nitems = cp.nitems; pd.use2d = cp.use2d; pd.profile = profile; pd.nout_words = nout_words; pd.h0 = h0; pd.h1 = h1;
  pd.arm_helpers = ctx->arm_helpers && ctx->host_split && ctx->horner_threads > 1 && cp.n <= ((size_t)1 << 18);
  return CG1_OK;
}

// The status record behind a call's exported points: [0] a scalar was >= 2^255, [1] entries sorted, [2] chunks k_accumulate ran (k_msm_small: none).
static int read_status_words(Ctx* ctx, const PointWords* record, bool has_chunks = true) {
  const uint32_t* st_words = reinterpret_cast<const uint32_t*>(record);
  ctx->last_entries = st_words[1]; ctx->last_chunks = has_chunks ? st_words[2] : 0;
  if (!st_words[0]) return CG1_OK;
  snprintf(ctx->err, sizeof ctx->err, "a scalar is >= 2^255: scalar32 must be a canonical Fr element (< r)");
  return CG1_ERR_ENCODING;
}

// The exported points of a call with their exponents, sorted by exponent for ONE Horner over global bit positions:
//   result = sum over the exported points P of 2^e(P) P, with (window w of the plan starts at bit off[w]):
//   2-D reduction:  e(T0_w) = off[w];  e(column bit k) = off[w] + k (k < lb);  e(row bit k) = off[w] + lb + k (k < hb)
//   1-D fallback:   e(T_w) = off[w];   e(Y_{w,b}) = off[w] + log2(m) + b
// (a window narrower than cmax leaves its top row bits empty: their points are the identity and are skipped)
struct HornerItems {
  static constexpr int EMAX = 2 * 256 + 64;
  std::vector<std::pair<int, const PointWords*>> items;          // (exponent, point) as put
  std::vector<const PointWords*> byexp;                          // grouped by exponent: those of weight 2^e are byexp[first[e] .. first[e + 1])
  uint16_t first[EMAX + 1];
  int e_top = 0;
  void put(int e, const PointWords* p) { if (!p->inf && e >= 0 && e < EMAX) { items.emplace_back(e, p); if (e > e_top) e_top = e; } }      // (a plan never leaves [0, EMAX): the guard keeps a planner bug off the stack)
  void put_2d(const PointWords* row, int base, uint32_t hb2, uint32_t lb2) {      // one window's 1 + hb + lb items
    put(base, &row[0]);
    for (uint32_t k = 0; k < hb2; ++k) put(base + (int)lb2 + (int)k, &row[1 + k]);
    for (uint32_t k = 0; k < lb2; ++k) put(base + (int)k, &row[1 + hb2 + k]);
  }
  void sort() {                                                  // counting sort by exponent
    memset(first, 0, sizeof first);
    for (const auto& it : items) ++first[it.first + 1];
    for (int e = 0; e < EMAX; ++e) first[e + 1] = (uint16_t)(first[e + 1] + first[e]);
    byexp.resize(items.size());
    uint16_t cur[EMAX];
    memcpy(cur, first, sizeof cur);
    for (const auto& it : items) byexp[cur[it.first]++] = it.second;
  }
  // horner(lo, hi) = sum_{e in [lo, hi]} 2^(e - lo) * (points of weight 2^e)
  cg1h::jac horner(int lo, int hi) const {
    cg1h::jac a = cg1h::jac_identity();
    for (int e = hi; e >= lo; --e) {
      a = cg1h::jac_dbl(a);
      for (uint16_t k = first[e]; k < first[e + 1]; ++k) a = cg1h::jac_add(a, jac_from_words(*byexp[k]));
    }
    return a;
  }
};

// Wait for what msm_enqueue queued on this context, then the host Horner tail over its windows.
static int msm_finish(Ctx* ctx, cg1h::jac& result) {
  result = cg1h::jac_identity();
  if (!ctx->pend.active) return CG1_OK;
  const Ctx::Pending pd = ctx->pend;
  ctx->pend.active = false;
  HIPCHK(hipSetDevice(ctx->device));
  // helpers armed below spin for a job for up to 2 ms: on every way out of this function (a failed stream, a bad scalar, a tail that needs
  // fewer threads) the ones still spinning are told to stand down
  struct StandDown { Ctx* c; bool on; ~StandDown() { if (on) for (int j = 0; j < 3; ++j) c->helper[j].disarm(); } } stand_down{ctx, false};
  if (pd.zero_copy && !ctx->blocking_sync && pd.profile < 2) {
    if (pd.arm_helpers) for (int j = 0; j < 3 && j + 1 < ctx->horner_threads; ++j) ctx->helper[j].arm();
    stand_down.on = pd.arm_helpers;
    int wrc = wait_export_flag(ctx, pd.seq); if (wrc) return wrc;
  } else {
    int wrc = wait_stream(ctx); if (wrc) return wrc;
  }
  HIPCHK(hipGetLastError());
  { int src = read_status_words(ctx, pd.hout + pd.nout_words); if (src) return src; }
  auto h2 = std::chrono::steady_clock::now();
  { int erc = read_phase_events(ctx, pd.profile); if (erc) return erc; }
  ctx->last_c = pd.c;
  auto t0 = std::chrono::steady_clock::now();
  ctx->host_ms[0] = std::chrono::duration<float, std::milli>(pd.h1 - pd.h0).count();
  ctx->host_ms[1] = std::chrono::duration<float, std::milli>(h2 - pd.h1).count();
  ctx->host_ms[2] = std::chrono::duration<float, std::milli>(t0 - h2).count();
  HornerItems hi;
  hi.items.reserve((size_t)pd.nlw * pd.nitems);
  int lm = 0; while ((1u << lm) < pd.m) ++lm;
  for (int lw = 0; lw < pd.nlw; ++lw) {
    const int base = pd.plan.off(win_global(lw, pd.rank, pd.world));
    const PointWords* row = pd.hout + (size_t)lw * pd.nitems;
    if (pd.use2d) { hi.put_2d(row, base, pd.hb2, pd.lb2); continue; }
    hi.put(base, &row[0]);
    for (int b2 = 0; b2 < pd.nbits; ++b2) hi.put(base + lm + b2, &row[1 + b2]);
  }
  hi.sort();
  const int e_top = hi.e_top;
  const uint16_t* first = hi.first;
  auto horner = [&](int lo, int hi_e) { return hi.horner(lo, hi_e); };
  cg1h::jac acc;
  const int nth = host_horner_threads(*ctx, e_top);
  ctx->last_tail = tail_with_horner(ctx->last_tail, HORNER_HOST, (uint32_t)nth);
  if (nth > 1) {
    // the exponent range cut into nth parts: part j (on its own thread) forms horner(lo_j, hi_j) and then doubles it lo_j times, so
    // every part ends with its full weight and the parts are simply added.  The critical path is the top part: e_top doublings,
    // but only a fraction of the additions.
    // The cut is NOT even: part j costs (lo_{j+1}) doublings + its own additions, so the top part gets the narrowest range.  With a
    // doubling at 7 and an addition at 16 field-multiplication times the largest part cost C is found by bisection (parts filled from
    // the bottom up to C each): four threads end ~18 % sooner than with equal ranges (255 doublings + ~40 additions on the top part).
    cg1h::jac part[4];
    int lo[5];
    {
      constexpr long DBL = 7, ADD = 16;
      auto fill = [&](long C, int* cut) {                          // greedy cut for a part-cost limit C; true if nth parts suffice
        int e = 0;
        for (int j = 0; j < nth; ++j) {
          cut[j] = e;
          long adds = 0;
          while (e <= e_top && DBL * (e + 1) + ADD * (adds + (first[e + 1] - first[e])) <= C) { adds += first[e + 1] - first[e]; ++e; }
        }
        cut[nth] = e_top + 1;
        return e > e_top;
      };
      long lo_c = DBL * (e_top + 1), hi_c = DBL * (e_top + 1) + ADD * (long)hi.items.size();
      int cut[5];
      while (lo_c < hi_c) {
        const long mid = (lo_c + hi_c) / 2;
        if (fill(mid, cut)) hi_c = mid; else lo_c = mid + 1;
      }
      fill(hi_c, cut);
      for (int j = 0; j <= nth; ++j) lo[j] = cut[j];
    }
    auto run_part = [&](int j) {
      cg1h::jac a = horner(lo[j], lo[j + 1] - 1);
      for (int k = 0; k < lo[j]; ++k) a = cg1h::jac_dbl(a);
      part[j] = a;
    };
    for (int j = 0; j + 1 < nth; ++j) ctx->helper[j].run([&, j]() { run_part(j); });
    if (pd.arm_helpers) for (int j = nth - 1 < 0 ? 0 : nth - 1; j < 3; ++j) ctx->helper[j].disarm();      // armed for a wider tail than this call has
    run_part(nth - 1);
    acc = part[nth - 1];
    for (int j = 0; j + 1 < nth; ++j) { ctx->helper[j].wait(); acc = cg1h::jac_add(acc, part[j]); }
  } else {
    if (pd.arm_helpers) for (int j = 0; j < 3; ++j) ctx->helper[j].disarm();
    acc = horner(0, e_top);
  }
  result = acc;
  ctx->host_tail_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  ctx->host_ms[3] = ctx->host_tail_ms;
  return CG1_OK;
}

// One launch (two when un-normalised blobs have to be inverted first) for an MSM of n <= SM_MAX_N terms -- or for M <= SM_MAX_MSMS
// independent ones of at most max_n terms each (d_offs: their M + 1 term offsets on the device); fills ctx->pend like msm_enqueue, so
// msm_finish polls the same flag and runs the same host Horner (M = 1), or msm_small_batched_finish does (M > 1).
static int msm_enqueue_small(Ctx* ctx, const PtSrc& src, const void* d_scalars32, size_t n, int c, uint32_t M = 1, const uint32_t* d_offs = nullptr, size_t max_n = 0,
                             bool glv = false) {
  ctx->pend.active = false;
  HIPCHK(hipSetDevice(ctx->device));
  const WinPlan plan = make_plan(c, glv);
  const uint32_t nwin = (uint32_t)plan.nwin, bb = (uint32_t)c - 1u, lb2 = (bb + 1u) / 2u, hb2 = bb - lb2, nitems = 1u + hb2 + lb2;
  if (M == 1) max_n = n;
  const uint32_t S = (uint32_t)(((glv ? 2 * max_n : max_n) + SM_SLICE - 1) / SM_SLICE);      // (split: slices of the 2n entries)
  auto h0 = std::chrono::steady_clock::now();
  if (!ctx->h_small_out) {
    HIPCHK(hipHostMalloc((void**)&ctx->h_small_out, ((size_t)SM_MAX_MSMS * 64 * 9 + 1) * sizeof(PointWords), hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer((void**)&ctx->h_small_out_dev, ctx->h_small_out, 0));
    HIPCHK(hipMalloc(&ctx->d_small_ctr, (SM_MAX_MSMS * 64 + 8) * 4));
    // on the context's own stream: it is a non-blocking stream, which a memset on the null stream would NOT be ordered with -- the
    // first launch could find its tickets zeroed under its feet ("the stream drained without the export flag")
    HIPCHK(hipMemsetAsync(ctx->d_small_ctr, 0, (SM_MAX_MSMS * 64 + 8) * 4, ctx->stream));
  }
  const size_t need_partial = (size_t)M * nwin * S * nitems;
  if (S > 1) { const int rc = grow_device(ctx, ctx->d_small_partial, ctx->cap_small_partial, need_partial, need_partial); if (rc) return rc; }
  hipStream_t st = ctx->stream;
  SmallArgs a;
  a.src = src.p; a.flags = src.flags; a.scalars = static_cast<const uint32_t*>(d_scalars32); a.offs = d_offs;
  a.n = (uint32_t)n; a.M = M; a.S = S; a.c = (uint32_t)c; a.nwin = nwin; a.hb = hb2; a.lb = lb2; a.nitems = nitems;
  a.partial = ctx->d_small_partial; a.counters = ctx->d_small_ctr;
  a.out_host = ctx->h_small_out_dev; a.flag_host = ctx->h_flag_dev; a.seq = ++ctx->seq;
  a.row_tail = ctx->small_row_tail ? 1u : 0u;
  ctx->last_tail = tail_word(small_tail(*ctx));
  a.glv = glv ? 1u : 0u;
  int kind = (int)src.kind;
  if (src.kind == PtSrc::BLOBS && !src.normalised) {           // invert first (one lane per point), then run on the prepared records
    const size_t cap = n < SM_MAX_N ? SM_MAX_N : n;
    { const int rc = grow_bufs(ctx, ctx->cap_small_pts, n, cap, {dev_buf(ctx->d_small_pts, cap * sizeof(PreparedPoint)), dev_buf(ctx->d_small_flags, cap + 16)}); if (rc) return rc; }
    launch_prepare(st, src, ctx->d_small_pts, ctx->d_small_flags, (uint32_t)n, nullptr);
    a.src = ctx->d_small_pts; a.flags = ctx->d_small_flags;
    kind = (int)PtSrc::PREPARED;
  }
  const dim3 grid(nwin, S, M), block(512);
  if (kind == (int)PtSrc::AFFINE96) hipLaunchKernelGGL((k_msm_small<0>), grid, block, 0, st, a);
  else if (kind == (int)PtSrc::BLOBS) hipLaunchKernelGGL((k_msm_small<1>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((k_msm_small<2>), grid, block, 0, st, a);
  auto h1 = std::chrono::steady_clock::now();
  Ctx::Pending& pd = ctx->pend;
  pd.zero_copy = true; pd.seq = ctx->seq; pd.hout = ctx->h_small_out;
  pd.active = true; pd.c = c; pd.plan = plan; pd.rank = 0; pd.world = 1; pd.nlw = (int)nwin; pd.nbits = 0; pd.m = 1; pd.lb2 = lb2; pd.hb2 = hb2;
  pd.nitems = nitems; pd.use2d = true; pd.profile = 0; pd.nout_words = (size_t)M * nwin * nitems; pd.h0 = h0; pd.h1 = h1;
  pd.arm_helpers = ctx->arm_helpers && ctx->host_split && ctx->horner_threads > 1 && M == 1;
  return CG1_OK;
}

// sum over a window-major block of exported 2-D items (1 + hb + lb per window, uniform plan) of 2^e(P) P: one Horner from the top bit
static cg1h::jac horner_2d_items(const PointWords* rows, const WinPlan& plan, uint32_t nitems, uint32_t hb2, uint32_t lb2) {
  HornerItems hi;
  hi.items.reserve((size_t)plan.nwin * nitems);
  for (int w = 0; w < plan.nwin; ++w) hi.put_2d(rows + (size_t)w * nitems, plan.off(w), hb2, lb2);
  hi.sort();
  return hi.horner(0, hi.e_top);
}

// Wait for a launch of M > 1 small MSMs and run their M host Horners (one thread each, up to four at a time).
static int msm_small_batched_finish(Ctx* ctx, uint32_t M, std::vector<cg1h::jac>& results) {
  const Ctx::Pending pd = ctx->pend;
  ctx->pend.active = false;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->blocking_sync) {
    int wrc = wait_export_flag(ctx, pd.seq); if (wrc) return wrc;
  } else {
    int wrc = wait_stream(ctx); if (wrc) return wrc;
  }
  HIPCHK(hipGetLastError());
  { int src = read_status_words(ctx, pd.hout + pd.nout_words, false); if (src) return src; }
  auto t0 = std::chrono::steady_clock::now();
  const size_t per = (size_t)pd.plan.nwin * pd.nitems;
  auto one = [&](size_t j) { results[j] = horner_2d_items(pd.hout + j * per, pd.plan, pd.nitems, pd.hb2, pd.lb2); };
  if (M <= 4) {
    const size_t nth = std::min<size_t>(4, M);
    for (size_t t = 1; t < nth; ++t) ctx->helper[t - 1].run([&, t]() { for (size_t j = t; j < M; j += nth) one(j); });
    for (size_t j = 0; j < M; j += nth) one(j);
    for (size_t t = 1; t < nth; ++t) ctx->helper[t - 1].wait();
  } else {                                             // more Horners than the context's own helpers: the process's worker pool, one Horner at a time per thread
    cg1::pool_for(M, 0, one);
  }
  ctx->last_tail = tail_with_horner(ctx->last_tail, HORNER_HOST, small_horner_threads(*ctx, M, 0));
  auto t1 = std::chrono::steady_clock::now();
  ctx->host_ms[0] = std::chrono::duration<float, std::milli>(pd.h1 - pd.h0).count();
  ctx->host_ms[1] = std::chrono::duration<float, std::milli>(t0 - pd.h1).count();
  ctx->host_ms[2] = 0;
  ctx->host_ms[3] = ctx->host_tail_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
  for (int i = 0; i < CG1_NPHASE; ++i) ctx->phase_ms[i] = 0.f;
  ctx->last_c = pd.c;
  ctx->last_acc_launches = 0;
  return CG1_OK;
}

static Ctx* child_of(Ctx* ctx);
static int msm_begin_split(Ctx* ctx, const PtSrc& src, const void* d_scalars32, size_t n, const WinPlan& plan, int rank, int world);

// One MSM: this context's share (windows w = rank mod world) of sum_i scalar_i * point_i.
// c = 0: automatic plan; 4..16: uniform windows of that width; -16..-4: the balanced plan with cmax = -c.
// msm_begin enqueues the whole launch chain and returns; msm_end waits for it and runs the host tail.  Two contexts on one
// GPU can thus keep two MSMs in flight: the sort phases of the next one run under this one's k_accumulate (they need few
// registers and co-reside with its waves), and this one's reduction tree, D2H and host Horner run under the next one's.
int msm_begin(Ctx* ctx, const PtSrc& src, const void* d_scalars32, size_t n, int c, int rank, int world) {
  ctx->pend.active = false;
  ctx->pend_c = 0;
  ctx->last_entries = ctx->last_chunks = 0; ctx->last_tail = 0;          // a call that enqueues nothing (no terms, a shard without a window) sorted nothing
  const Route r = route_msm_call(*ctx, n, c, rank, world, (int)src.kind);
  if (r.rc) { snprintf(ctx->err, sizeof ctx->err, "%s", r.err); return r.rc; }
  ctx->pend_c = r.c;
  switch (r.engine) {
    case ENGINE_NONE: return CG1_OK;
    case ENGINE_SMALL: return msm_enqueue_small(ctx, src, d_scalars32, n, r.c, 1, nullptr, 0, r.glv);
    case ENGINE_TWO_CHAINS_A: ctx->pend_split = false; return msm_begin_split(ctx, src, d_scalars32, n, r.plan, rank, world);
    default: ctx->pend_split = false; return msm_enqueue(ctx, src, d_scalars32, n, r.plan, rank, world);
  }
}
int msm_end(Ctx* ctx, cg1h::jac& result) {
  const bool was_small = ctx->pend.active && ctx->pend.hout == ctx->h_small_out;
  int rc = msm_finish(ctx, result);                    // (split: the HIGH windows; their Horner runs while the GPU is still on the low half)
  ctx->last_acc_launches = ctx->pend_split ? 2 : (was_small ? 0 : 1);
  if (ctx->pend_split) {
    ctx->pend_split = false;
    Ctx* ch = child_of(ctx);
    const float acc_hi = ctx->phase_ms[4], wait_hi = ctx->host_ms[1], tail_hi = ctx->host_ms[3], enq = ctx->host_ms[0];
    const uint32_t e_hi = ctx->last_entries, c_hi = ctx->last_chunks;
    cg1h::jac lo;
    int rc2 = msm_finish(ch, lo);
    if (rc == CG1_OK) rc = rc2;
    if (rc2 != CG1_OK) snprintf(ctx->err, sizeof ctx->err, "%s", ch->err);
    if (rc == CG1_OK) result = cg1h::jac_add(result, lo);
    // the call's figures: both k_accumulate launches, both chains' entries; host: enqueue of both chains, waits, tails
    for (int i = 0; i < CG1_NPHASE; ++i) ctx->phase_ms[i] += ch->phase_ms[i];
    ctx->phase_ms[4] = acc_hi + ch->phase_ms[4];
    ctx->last_entries = e_hi + ch->last_entries; ctx->last_chunks = c_hi + ch->last_chunks;
    ctx->host_ms[0] = enq + ch->host_ms[0]; ctx->host_ms[1] = wait_hi + ch->host_ms[1]; ctx->host_ms[3] = tail_hi + ch->host_ms[3];
    ctx->host_tail_ms = ch->host_ms[3];                 // what is left on the critical path after the GPU is done
  }
  if (ctx->pend_c) ctx->last_c = ctx->pend_c;          // negative: a balanced plan (cg1_get_timings reports it)
  return rc;
}
int msm_device(Ctx* ctx, const PtSrc& src, const void* d_scalars32, size_t n, int c, int rank, int world, cg1h::jac& result) {
  result = cg1h::jac_identity();
  int rc = msm_begin(ctx, src, d_scalars32, n, c, rank, world);
  if (rc) return rc;
  return msm_end(ctx, result);
}


static int ensure_child(Ctx* ctx);      // the second launch chain's context and the two events between the chains (capi_core_msm.h)

// The regime-B launch chain of one (sub-)batch, in two steps so that two of them can be in flight (msm_batched_device below):
// batched_chain_enqueue queues everything up to the D2H of the results and returns; batched_chain_finish waits and reads them back.
struct BatchedChain {
  size_t M = 0; int c = 0; uint32_t nwin = 0; bool host_horner = false;
  std::chrono::steady_clock::time_point h0, h1;
};
static int batched_chain_enqueue(Ctx* ctx, const void* d_points96, const void* d_scalars32, const uint32_t* h_offsets, size_t M, int c, bool glv,
                                 hipEvent_t wait_before_accumulate, hipEvent_t record_after_accumulate, BatchedChain& bc) {
  const size_t N = h_offsets[M];
  HIPCHK(hipSetDevice(ctx->device));
  const BatchPlan bp = plan_regime_b(*ctx, M, N, c, glv);
  if (bp.rc) { snprintf(ctx->err, sizeof ctx->err, "batch too large"); return bp.rc; }
  const uint32_t nwin = bp.nwin, NB = bp.NB;
  const size_t G = bp.G, Nv = bp.Nv;
  int rc = ensure(ctx, Nv, bp.nb_total, nwin, 1, bp.L);
  if (rc) return rc;
  // batch-only buffers
  if ((rc = grow_device(ctx, ctx->d_boffs, ctx->cap_boffs, M + 1, M + 1))) return rc;
  if ((rc = grow_device(ctx, ctx->d_gsum, ctx->cap_gsum, G, G))) return rc;
  if ((rc = grow_bufs(ctx, ctx->cap_bout, M, M, {dev_buf(ctx->d_bout, (M + 1) * sizeof(PointWords)),         // + one record: the input-validation flag word
                                                 host_buf(ctx->h_bout, (M + 1) * sizeof(PointWords))}))) return rc;
  if ((rc = grow_bufs(ctx, ctx->cap_digits, Nv * nwin, Nv * nwin, {dev_buf(ctx->d_digits, Nv * nwin * 2 + 16)}))) return rc;
  if (bp.host_horner && (rc = grow_bufs(ctx, ctx->cap_gout, G, G, {dev_buf(ctx->d_gout, G * sizeof(PointWords)), host_buf(ctx->h_gout, G * sizeof(PointWords))}))) return rc;
  hipStream_t st = ctx->stream;
  const uint32_t N32 = (uint32_t)N, gn = (N32 + 255) / 256, Nv32 = (uint32_t)Nv, split = glv ? N32 : 0u;
  auto h0 = std::chrono::steady_clock::now();
  HIPCHK(hipMemcpyAsync(ctx->d_boffs, h_offsets, (M + 1) * 4, hipMemcpyHostToDevice, st));
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[0], st));
  uint32_t* bad_flag = reinterpret_cast<uint32_t*>(ctx->d_bout + M);
  hipLaunchKernelGGL(k_prepare_points, dim3(gn), dim3(256), 0, st, (const uint32_t*)d_points96, ctx->d_pts, ctx->d_flags, N32, bad_flag);
  if (glv) hipLaunchKernelGGL(k_phi_records, dim3(gn), dim3(256), 0, st, ctx->d_pts, ctx->d_flags, N32);
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[1], st));
  hipLaunchKernelGGL(k_digits, dim3(gn), dim3(256), 0, st, (const uint32_t*)d_scalars32, ctx->d_flags, ctx->d_digits, N32, bp.plan, 0, 1, bad_flag);
  hipLaunchKernelGGL(k_group_count, dim3((uint32_t)M, nwin), dim3(256), 0, st, ctx->d_digits, ctx->d_boffs, ctx->d_hist, Nv32, NB, nwin, split);
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[2], st));
  stage_scan3(ctx, bp.nb_total, bp.L);
  hipLaunchKernelGGL(k_group_scatter, dim3((uint32_t)M, nwin), dim3(256), 0, st, ctx->d_digits, ctx->d_boffs, ctx->d_off, ctx->d_sorted, Nv32, NB, nwin, split);
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[3], st));
  if ((rc = stage_accumulate(ctx, bp.nb_total, Nv * (size_t)nwin, bp.L, ctx->d_pts, bad_flag, wait_before_accumulate, record_after_accumulate))) return rc;
  const uint32_t nseg_total = (uint32_t)(bp.nb_total / bp.m);
  hipLaunchKernelGGL(k_seg_reduce, dim3((nseg_total + 255) / 256), dim3(256), 0, st, ctx->d_choff, ctx->d_sums, ctx->d_combined, ctx->d_segrun, ctx->d_segtot, nseg_total, bp.m);
  hipLaunchKernelGGL(k_group_reduce, dim3((uint32_t)((G + 255) / 256)), dim3(256), 0, st, ctx->d_segrun, ctx->d_segtot, ctx->d_gsum, (uint32_t)G, bp.J, bp.log2m);
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[6], st));
  if (bp.tail.horner == HORNER_HOST) {
    hipLaunchKernelGGL(k_export_sums, dim3((uint32_t)((G + 63) / 64)), dim3(64), 0, st, ctx->d_gsum, ctx->d_gout, (uint32_t)G);
    HIPCHK(hipMemcpyAsync(ctx->h_gout, ctx->d_gout, G * sizeof(PointWords), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ctx->h_bout + M, ctx->d_bout + M, sizeof(PointWords), hipMemcpyDeviceToHost, st));      // the status words
  } else {
    if (bp.tail.horner == HORNER_ROW) hipLaunchKernelGGL(k_msm_horner_row, dim3((uint32_t)M), dim3(64), 0, st, ctx->d_gsum, ctx->d_bout, (uint32_t)M, nwin, (uint32_t)c);
    else if (bp.tail.horner == HORNER_QUAD) hipLaunchKernelGGL(k_msm_horner_quad, dim3((uint32_t)((M * 4 + 63) / 64)), dim3(64), 0, st, ctx->d_gsum, ctx->d_bout, (uint32_t)M, nwin, (uint32_t)c);
    else hipLaunchKernelGGL(k_msm_horner, dim3((uint32_t)((M + 63) / 64)), dim3(64), 0, st, ctx->d_gsum, ctx->d_bout, (uint32_t)M, nwin, (uint32_t)c);
    HIPCHK(hipMemcpyAsync(ctx->h_bout, ctx->d_bout, (M + 1) * sizeof(PointWords), hipMemcpyDeviceToHost, st));
  }
  if (ctx->profile >= 2) HIPCHK(hipEventRecord(ctx->ev[7], st));
  ctx->last_tail = tail_word(bp.tail);
  bc.M = M; bc.c = c; bc.nwin = nwin; bc.host_horner = bp.host_horner; bc.h0 = h0; bc.h1 = std::chrono::steady_clock::now();
  return CG1_OK;
}

static int batched_chain_finish(Ctx* ctx, const BatchedChain& bc, cg1h::jac* results) {
  const size_t M = bc.M; const int c = bc.c; const uint32_t nwin = bc.nwin; const bool host_horner = bc.host_horner;
  const auto h0 = bc.h0, h1 = bc.h1;
  HIPCHK(hipSetDevice(ctx->device));
  { int wrc = wait_stream(ctx); if (wrc) return wrc; }
  HIPCHK(hipGetLastError());
  { int src = read_status_words(ctx, ctx->h_bout + M); if (src) return src; }
  auto h2 = std::chrono::steady_clock::now();
  { int erc = read_phase_events(ctx, ctx->profile); if (erc) return erc; }
  ctx->last_c = c;
  if (host_horner) {
    auto one = [&](size_t j) {
      cg1h::jac a = cg1h::jac_identity();
      for (int w = (int)nwin - 1; w >= 0; --w) {
        for (int k = 0; k < c; ++k) a = cg1h::jac_dbl(a);
        a = cg1h::jac_add(a, jac_from_words(ctx->h_gout[j * nwin + (size_t)w]));
      }
      results[j] = a;
    };
    const size_t nth = std::min<size_t>(4, M);
    for (size_t t = 1; t < nth; ++t) ctx->helper[t - 1].run([&, t]() { for (size_t j = t; j < M; j += nth) one(j); });
    for (size_t j = 0; j < M; j += nth) one(j);
    for (size_t t = 1; t < nth; ++t) ctx->helper[t - 1].wait();
  } else {
    for (size_t j = 0; j < M; ++j) results[j] = jac_from_words(ctx->h_bout[j]);
  }
  auto h3 = std::chrono::steady_clock::now();
  ctx->host_ms[0] = std::chrono::duration<float, std::milli>(h1 - h0).count();
  ctx->host_ms[1] = std::chrono::duration<float, std::milli>(h2 - h1).count();
  ctx->host_ms[2] = 0;
  ctx->host_ms[3] = ctx->host_tail_ms = std::chrono::duration<float, std::milli>(h3 - h2).count();
  return CG1_OK;
}

// M independent MSMs over one concatenated (points, scalars) input resident on the device.
// async_small (may be NULL): when the call fits ONE k_msm_small launch it is only ENQUEUED and *async_small set; the caller does other
// work and collects the results with msm_batched_small_end.  Calls that take the regime-B chain complete before returning.
static int msm_batched_small_end(Ctx* ctx, size_t M, std::vector<cg1h::jac>& results) {
  if (M == 1) { cg1h::jac r; int rc = msm_finish(ctx, r); ctx->last_acc_launches = 0; if (rc == CG1_OK) results[0] = r; return rc; }
  return msm_small_batched_finish(ctx, (uint32_t)M, results);
}
// d_offsets_ready (may be NULL): the same M + 1 offsets at an address the DEVICE can read (mapped host memory); the single-launch path
// then reads them there instead of waiting for a copy.
int msm_batched_device(Ctx* ctx, const void* d_points96, const void* d_scalars32, const uint32_t* h_offsets, size_t M,
                       int c, std::vector<cg1h::jac>& results, bool* async_small = nullptr, const uint32_t* d_offsets_ready = nullptr) {
  if (async_small) *async_small = false;
  results.assign(M, cg1h::jac_identity());
  if (M == 0) return CG1_OK;
  const size_t N = h_offsets[M];
  for (size_t j = 0; j < M; ++j) if (h_offsets[j] > h_offsets[j + 1]) { snprintf(ctx->err, sizeof ctx->err, "offsets not monotone"); return CG1_ERR_ARG; }
  if (h_offsets[0] != 0) { snprintf(ctx->err, sizeof ctx->err, "offsets[0] must be 0"); return CG1_ERR_ARG; }
  size_t max_n = 0;
  for (size_t j = 0; j < M; ++j) max_n = std::max<size_t>(max_n, h_offsets[j + 1] - h_offsets[j]);
  const Route r = route_batched_call(*ctx, M, N, max_n, c, h_offsets[M / 2] == 0 || h_offsets[M / 2] == N);
  if (r.rc) { snprintf(ctx->err, sizeof ctx->err, "%s", r.err); return r.rc; }
  if (r.engine == ENGINE_NONE) return CG1_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (r.engine == ENGINE_SMALL) {
    const uint32_t* d_offs = d_offsets_ready;
    if (!d_offs) {
      { const int rc = grow_device(ctx, ctx->d_boffs, ctx->cap_boffs, M + 1, M + 1); if (rc) return rc; }
      HIPCHK(hipMemcpyAsync(ctx->d_boffs, h_offsets, (M + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
      d_offs = ctx->d_boffs;
    }
    int rc = msm_enqueue_small(ctx, PtSrc(d_points96), d_scalars32, N, r.c, (uint32_t)M, d_offs, max_n, r.glv);
    if (rc) return rc;
    if (async_small) { *async_small = true; return CG1_OK; }
    return msm_batched_small_end(ctx, M, results);
  }
  c = r.c;
  const bool glv = r.glv;
  if (r.engine == ENGINE_CHAIN_B) {
    BatchedChain bc;
    int rc = batched_chain_enqueue(ctx, d_points96, d_scalars32, h_offsets, M, c, glv, nullptr, nullptr, bc);
    if (rc) return rc;
    return batched_chain_finish(ctx, bc, results.data());
  }
  // Two chains, half the MSMs each, on two streams: the second half's k_accumulate starts when the first half's has finished, so the
  // first half's latency-bound tail (group sums, one wave per MSM for 255 doublings, D2H) runs UNDER the second half's additions
  // instead of after them.  ("batched_split", default off: measured slower, profiles/r05_regime_b_split.txt.)
  { int crc = ensure_child(ctx); if (crc) return crc; }
  Ctx* ch = child_of(ctx);
  const size_t Mlo = M / 2, Mhi = M - Mlo;
  std::vector<uint32_t> offs_hi(Mhi + 1);
  for (size_t j = 0; j <= Mhi; ++j) offs_hi[j] = h_offsets[Mlo + j] - h_offsets[Mlo];
  BatchedChain lo, hi;
  int rc = batched_chain_enqueue(ctx, d_points96, d_scalars32, h_offsets, Mlo, c, glv, nullptr, ctx->ev_acc, lo);
  if (rc) return rc;
  rc = batched_chain_enqueue(ch, static_cast<const uint8_t*>(d_points96) + 96ull * h_offsets[Mlo], static_cast<const uint8_t*>(d_scalars32) + 32ull * h_offsets[Mlo],
                             offs_hi.data(), Mhi, c, glv, ctx->ev_acc, nullptr, hi);
  if (rc) { snprintf(ctx->err, sizeof ctx->err, "%s", ch->err); (void)batched_chain_finish(ctx, lo, results.data()); return rc; }
  rc = batched_chain_finish(ctx, lo, results.data());
  const float acc_lo = ctx->phase_ms[4], enq_lo = ctx->host_ms[0], wait_lo = ctx->host_ms[1];
  const uint32_t e_lo = ctx->last_entries, c_lo = ctx->last_chunks;
  int rc2 = batched_chain_finish(ch, hi, results.data() + Mlo);
  if (rc2 != CG1_OK) snprintf(ctx->err, sizeof ctx->err, "%s", ch->err);
  if (rc == CG1_OK) rc = rc2;
  ctx->phase_ms[4] = acc_lo + ch->phase_ms[4];
  ctx->last_entries = e_lo + ch->last_entries; ctx->last_chunks = c_lo + ch->last_chunks;
  ctx->host_ms[0] = enq_lo + ch->host_ms[0]; ctx->host_ms[1] = wait_lo + ch->host_ms[1];
  return rc;
}

}  // namespace cg1
