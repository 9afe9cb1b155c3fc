// C ABI, part 8: resident tables of fixed bases and the MSMs over them (kernels_fixed.h).
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

// What the MSM calls over a table share, whatever its records are (k_table_msm's plans: kernels_fixed.h, kernels_light.h).
struct cg1_table {
  int device = 0;
  size_t n_bases = 0;
  uint32_t* d_ctr = nullptr;                                // FX_MAX_MSMS + 8 words: tickets, finished MSMs, status bits; zero between calls
  uint32_t* d_status = nullptr;                             // 4 words: the status of a call that exports on the device only
  cg1::PointSum* d_partial = nullptr; size_t cap_partial = 0;
  cg1::PointSum* d_sum = nullptr;                           // FX_MAX_MSMS records for k_fixed_finish
  cg1::PointWords* h_out = nullptr; cg1::PointWords* h_out_dev = nullptr;      // pinned + mapped: FX_MAX_MSMS records + the status record
  uint8_t* h_in = nullptr; uint8_t* h_in_dev = nullptr; uint8_t* d_in = nullptr; size_t cap_in = 0;   // offsets | indices | scalars of a host call

  // everything but the records and the staging of a host call; the words are zeroed on the context's own (non-blocking) stream, like
  // k_msm_small's tickets: a null-stream memset is not ordered with it.  Nothing waits here.
  int alloc(cg1_ctx* ctx) {
    HIPCHK(hipMalloc(&d_ctr, (cg1::FX_MAX_MSMS + 8) * 4));
    HIPCHK(hipMalloc(&d_status, 16));
    HIPCHK(hipMalloc(&d_sum, (size_t)cg1::FX_MAX_MSMS * sizeof(cg1::PointSum)));
    HIPCHK(hipHostMalloc((void**)&h_out, ((size_t)cg1::FX_MAX_MSMS + 1) * sizeof(cg1::PointWords), hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer((void**)&h_out_dev, h_out, 0));
    HIPCHK(hipMemsetAsync(d_ctr, 0, (cg1::FX_MAX_MSMS + 8) * 4, ctx->stream));
    HIPCHK(hipMemsetAsync(d_status, 0, 16, ctx->stream));
    return CG1_OK;
  }
  void release() {
    cg1::release_bufs({cg1::dev_buf(d_ctr), cg1::dev_buf(d_status), cg1::dev_buf(d_sum), cg1::host_buf(h_out, 0, 0u, &h_out_dev)});
    cg1::release_bufs(cap_partial, {cg1::dev_buf(d_partial)});
    cg1::release_bufs(cap_in, {cg1::host_buf(h_in, 0, 0u, &h_in_dev), cg1::dev_buf(d_in)});
  }
};

struct cg1_fixed : cg1_table {
  cg1::PreparedPoint* d_tab = nullptr;                      // n_bases x GEN_ENTRIES records (build_fixed_table)
  uint8_t* h_chain = nullptr; uint8_t* d_chain = nullptr; size_t cap_chain = 0;      // the device provers' staging block and its device twin, re-laid-out by every call (capi_chain.h)
  size_t chain_used = 0;                // the largest layout of that block since a caller last reset it: what a call that wipes it has to cover
  cg1_light* smsm_light = nullptr; size_t cap_smsm_bases = 0;                  // the light table a device prover builds over per-proof bases (chain_light_scratch, capi_light.h): regrown only when too small
};

namespace {
constexpr size_t FX_ZERO_COPY_MAX = 256 * 1024;             // bytes of a host call's arguments the kernel reads straight from mapped host memory

// A kind of table on the host side: its handle, its plan of k_table_msm, and the data the shared functions below differ by.
struct FixedKind {
  using Handle = cg1_fixed;
  using Plan = cg1::FixedPlan;
  static constexpr const char* WHAT = "fixed-base MSM";     // error texts
  static constexpr const char* ENTRY = "cg1_fixed_msm";
  static constexpr uint32_t MAX_MSMS = cg1::FX_MAX_MSMS, MAX_TERMS = cg1::FX_MAX_TERMS;
  static constexpr uint32_t FIRST_SLICE = 2, SLICE_8_WAVES = 4;      // table_pick_shape
};

int fixed_create_impl(cg1_ctx* ctx, cg1_fixed* t, const uint8_t* bases96, size_t m) {
  for (size_t b = 0; b < m; ++b) {                          // canonical coordinates, on the curve (or the all-zero identity record)
    uint8_t blob[CG1_POINT_BYTES];
    const int rc = cg1_from_affine96(blob, bases96 + 96 * b, 1);
    if (rc != CG1_OK) { snprintf(ctx->err, sizeof ctx->err, "fixed base %zu: not a curve point (status %d)", b, rc); return rc; }
  }
  HIPCHK(hipSetDevice(ctx->device));
  { const int rc = build_fixed_table(ctx, bases96, m, &t->d_tab); if (rc) return rc; }
  { const int rc = t->alloc(ctx); if (rc) return rc; }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return CG1_OK;
}

// The launch shape of a call.  Every addition is a step of a dependent chain, and what a step costs is set by how many waves share a
// SIMD: 1.8 us alone, 2.5 us for two, ~4.5 us for four (profiles/r05_rowlane_ab.txt).  So: the smallest slice (terms per workgroup)
// that keeps the call within one round of the chip's 256 CUs -- the fewest dependent additions per wave -- and for such short slices
// (<= SLICE_8_WAVES) 8 waves per workgroup (two per SIMD) instead of 16; a call that cannot fit one round takes the longest slices
// (fewest partial sums to join).  groups(s) = workgroups at slice s.  The fixed tables start at 2 terms = 64 records; a light table's
// term is up to LT_WINDOWS additions, twice that at c = 4, so its slices start at ONE term -- the prover's shape, 4 MSMs of 64 terms, is
// then 256 workgroups of 8 waves, 8 dependent additions per wave and the tree.  "fixed_slice" / "fixed_waves" override for both kinds
// (A/B runs: tools/gpu_fixed_base_timing.py --shapes).
struct TableShape { uint32_t slice, waves; };
template <class K, typename F>
TableShape table_pick_shape(const cg1_ctx* ctx, F groups, uint32_t M, uint32_t max_terms) {
  TableShape sh{cg1::FX_MAX_SLICE, cg1::FX_WAVES};
  for (uint32_t s = K::FIRST_SLICE; s < cg1::FX_MAX_SLICE; s <<= 1)
    if (groups(s) <= 256) { sh.slice = s; break; }
  if (sh.slice <= K::SLICE_8_WAVES) sh.waves = 8;
  if (ctx->fixed_slice > 0 && (size_t)M * ((max_terms + ctx->fixed_slice - 1) / ctx->fixed_slice) <= 65536) sh.slice = (uint32_t)ctx->fixed_slice;
  if (ctx->fixed_waves > 0) sh.waves = (uint32_t)ctx->fixed_waves;
  return sh;
}
// ... of M MSMs of up to max_terms terms each, as the device entries and the launch chains size their grids
template <class K>
TableShape table_pick_shape(const cg1_ctx* ctx, uint32_t M, uint32_t max_terms) {
  return table_pick_shape<K>(ctx, [&](uint32_t s) { return (size_t)M * std::max<uint32_t>(1u, (max_terms + s - 1) / s); }, M, max_terms);
}

// enqueue k_table_msm (+ k_fixed_finish for device outputs); the term arrays are device-visible pointers
template <class K>
int table_enqueue(cg1_ctx* ctx, typename K::Handle* t, const uint32_t* d_tb, const uint32_t* d_sc, const uint32_t* d_offs, uint32_t M, uint32_t n_terms,
                  uint32_t max_terms, TableShape shape, bool to_host, void* d_out96, void* d_out48) {
  const uint32_t slice = shape.slice;
  const uint32_t Smax = max_terms ? (max_terms + slice - 1) / slice : 1u;
  const size_t need = (size_t)M * Smax;
  if (Smax > 1) { const int rc = cg1::grow_device(ctx, t->d_partial, t->cap_partial, need, need); if (rc) return rc; }
  cg1::TableArgs<typename K::Plan::Record> a;
  a.tab = t->d_tab; a.n_bases = (uint32_t)t->n_bases;
  a.term_base = d_tb; a.scalars = d_sc; a.offs = d_offs;
  a.M = M; a.n_terms = n_terms; a.max_terms = max_terms; a.slice = slice; a.Smax = Smax;
  a.partial = t->d_partial; a.counters = t->d_ctr;
  a.out_host = to_host ? t->h_out_dev : nullptr;
  a.status_out = to_host ? reinterpret_cast<uint32_t*>(t->h_out_dev + M) : t->d_status;
  a.flag_host = to_host ? ctx->h_flag_dev : nullptr;
  a.seq = to_host ? ++ctx->seq : 0u;
  a.out_sum = (d_out96 || d_out48) ? t->d_sum : nullptr;
  hipLaunchKernelGGL(cg1::k_table_msm<typename K::Plan>, dim3(Smax, M), dim3(shape.waves * 64), 0, ctx->stream, a);
  if (a.out_sum)
    hipLaunchKernelGGL(cg1::k_fixed_finish, dim3((M + 3) / 4), dim3(64), 0, ctx->stream, (const cg1::PointSum*)t->d_sum, (const uint32_t*)a.status_out, M,
                       (uint32_t*)d_out96, (uint32_t*)d_out48);
  return CG1_OK;
}

template <class K>
int table_status_error(cg1_ctx* ctx, uint32_t st) {
  if (st & cg1::FX_BAD_OFFSETS) { snprintf(ctx->err, sizeof ctx->err, "%s: offsets not ascending, past the term arrays, or an MSM longer than max_terms", K::WHAT); return CG1_ERR_ARG; }
  if (st & cg1::FX_BAD_INDEX) { snprintf(ctx->err, sizeof ctx->err, "%s: a term's base index is outside the table", K::WHAT); return CG1_ERR_ARG; }
  if (st & cg1::FX_BAD_SCALAR) { snprintf(ctx->err, sizeof ctx->err, "%s: a scalar is >= r: scalar32 must be a canonical Fr element", K::WHAT); return CG1_ERR_ENCODING; }
  return CG1_OK;
}

// the body of cg1_fixed_msm / cg1_light_msm
template <class K>
int table_msm_host(cg1_ctx* ctx, typename K::Handle* t, const uint32_t* term_base, const uint8_t* term_scalars32, const uint32_t* offsets, size_t n_msm,
                   uint8_t* out_blobs144, uint8_t* out_comp48) {
  if (!ctx) return CG1_ERR_HIP;
  if (n_msm == 0) return CG1_OK;
  if (!t || !offsets || (!out_blobs144 && !out_comp48) || t->device != ctx->device) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", K::ENTRY); return CG1_ERR_ARG; }
  if (n_msm > K::MAX_MSMS) { snprintf(ctx->err, sizeof ctx->err, "%s: more than %u MSMs in one call", K::ENTRY, K::MAX_MSMS); return CG1_ERR_ARG; }
  const uint32_t M = (uint32_t)n_msm;
  uint32_t max_terms = 0;
  if (offsets[0] != 0) { snprintf(ctx->err, sizeof ctx->err, "%s: offsets[0] must be 0", K::ENTRY); return CG1_ERR_ARG; }
  for (uint32_t j = 0; j < M; ++j) {
    if (offsets[j + 1] < offsets[j] || offsets[j + 1] - offsets[j] > K::MAX_TERMS) {
      snprintf(ctx->err, sizeof ctx->err, "%s: MSM %u: offsets not ascending or more than %u terms", K::ENTRY, j, K::MAX_TERMS);
      return CG1_ERR_ARG;
    }
    max_terms = std::max(max_terms, offsets[j + 1] - offsets[j]);
  }
  const uint32_t n = offsets[M];
  if (n && (!term_base || !term_scalars32)) { snprintf(ctx->err, sizeof ctx->err, "%s: bad argument", K::ENTRY); return CG1_ERR_ARG; }
  for (uint32_t i = 0; i < n; ++i) {                        // the whole call is refused before anything is written
    if ((term_base[i] & 0x7fffffffu) >= t->n_bases) return table_status_error<K>(ctx, cg1::FX_BAD_INDEX);
    uint32_t s[8];
    memcpy(s, term_scalars32 + 32 * (size_t)i, 32);
    if (!cg1::fixed_scalar_below_r(s)) return table_status_error<K>(ctx, cg1::FX_BAD_SCALAR);
  }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->pend.active = false;
  // one page-locked block: offsets | indices | scalars
  const size_t o_tb = ((size_t)(M + 1) * 4 + 15) & ~(size_t)15, o_sc = (o_tb + (size_t)n * 4 + 15) & ~(size_t)15, bytes = o_sc + (size_t)n * 32;
  { const int rc = cg1::grow_pinned_pair(ctx, t->h_in, &t->h_in_dev, t->d_in, t->cap_in, bytes, std::max<size_t>(bytes + bytes / 4, 64 * 1024),
                                         hipHostMallocMapped | hipHostMallocCoherent); if (rc) return rc; }
  memcpy(t->h_in, offsets, (size_t)(M + 1) * 4);
  if (n) { memcpy(t->h_in + o_tb, term_base, (size_t)n * 4); memcpy(t->h_in + o_sc, term_scalars32, (size_t)n * 32); }
  const uint8_t* src = t->h_in_dev;
  if (bytes > FX_ZERO_COPY_MAX) {
    HIPCHK(hipMemcpyAsync(t->d_in, t->h_in, bytes, hipMemcpyHostToDevice, ctx->stream));
    src = t->d_in;
  }
  const TableShape shape = table_pick_shape<K>(ctx, [&](uint32_t s) { size_t g = 0; for (uint32_t j = 0; j < M; ++j) g += std::max<uint32_t>(1u, (offsets[j + 1] - offsets[j] + s - 1) / s); return g; }, M, max_terms);
  { const int rc = table_enqueue<K>(ctx, t, (const uint32_t*)(src + o_tb), (const uint32_t*)(src + o_sc), (const uint32_t*)src, M, n, max_terms, shape, true, nullptr, nullptr); if (rc) return rc; }
  { const int rc = ctx->blocking_sync ? cg1::wait_stream(ctx) : cg1::wait_export_flag(ctx, ctx->seq); if (rc) return rc; }
  HIPCHK(hipGetLastError());
  { const int rc = table_status_error<K>(ctx, reinterpret_cast<const uint32_t*>(t->h_out + M)[0]); if (rc) return rc; }
  std::vector<uint8_t> tmp;
  uint8_t* blobs = out_blobs144;
  if (!blobs) { tmp.resize((size_t)M * CG1_POINT_BYTES); blobs = tmp.data(); }
  for (uint32_t j = 0; j < M; ++j) blob_out(blobs + (size_t)CG1_POINT_BYTES * j, cg1::jac_from_words(t->h_out[j]));
  if (out_comp48) cg1_batch_compress(out_comp48, blobs, M);
  return CG1_OK;
}

// the body of cg1_fixed_msm_device / cg1_light_msm_device
template <class K>
int table_msm_device(cg1_ctx* ctx, typename K::Handle* t, const void* d_term_base, const void* d_term_scalars32, const void* d_offsets, size_t n_msm,
                     size_t n_terms, size_t max_terms, void* d_out_affine96, void* d_out_comp48) {
  if (!ctx) return CG1_ERR_HIP;
  if (n_msm == 0) return CG1_OK;
  if (!t || !d_offsets || (!d_out_affine96 && !d_out_comp48) || t->device != ctx->device || (n_terms && (!d_term_base || !d_term_scalars32)) ||
      n_msm > K::MAX_MSMS || max_terms > K::MAX_TERMS || max_terms > n_terms || n_terms > (size_t)K::MAX_MSMS * K::MAX_TERMS) {
    snprintf(ctx->err, sizeof ctx->err, "%s_device: bad argument", K::ENTRY);
    return CG1_ERR_ARG;
  }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->pend.active = false;
  const uint32_t M = (uint32_t)n_msm, mt = (uint32_t)max_terms;
  { const int rc = table_enqueue<K>(ctx, t, (const uint32_t*)d_term_base, (const uint32_t*)d_term_scalars32, (const uint32_t*)d_offsets, M, (uint32_t)n_terms, mt,
                                    table_pick_shape<K>(ctx, M, mt), false, d_out_affine96, d_out_comp48); if (rc) return rc; }
  uint32_t st[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(st, t->d_status, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  return table_status_error<K>(ctx, st[0]);
}
}  // namespace

extern "C" {
cg1_fixed* cg1_fixed_create(cg1_ctx* ctx, const uint8_t* bases_affine96, size_t n_bases, int* status) {
  int rc = CG1_OK;
  cg1_fixed* t = nullptr;
  if (!ctx) rc = CG1_ERR_HIP;
  else if (!bases_affine96 || n_bases < 1 || n_bases > CG1_FIXED_MAX_BASES) { snprintf(ctx->err, sizeof ctx->err, "a fixed-base table holds 1 .. %d bases", CG1_FIXED_MAX_BASES); rc = CG1_ERR_ARG; }
  else {
    t = new cg1_fixed();
    t->device = ctx->device; t->n_bases = n_bases;
    rc = fixed_create_impl(ctx, t, bases_affine96, n_bases);
    if (rc != CG1_OK) { cg1_fixed_destroy(t); t = nullptr; }
  }
  if (status) *status = rc;
  return t;
}
void cg1_fixed_destroy(cg1_fixed* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  cg1::release_bufs({cg1::dev_buf(t->d_tab)});
  t->release();
  cg1::release_bufs(t->cap_chain, {cg1::host_buf(t->h_chain), cg1::dev_buf(t->d_chain)});
  if (t->smsm_light) cg1_light_destroy(t->smsm_light);
  delete t;
}
size_t cg1_fixed_len(const cg1_fixed* t) { return t ? t->n_bases : 0; }
size_t cg1_fixed_bytes(const cg1_fixed* t) { return t ? t->n_bases * (size_t)cg1::GEN_ENTRIES * sizeof(cg1::PreparedPoint) : 0; }

int cg1_fixed_msm(cg1_ctx* ctx, cg1_fixed* t, const uint32_t* term_base, const uint8_t* term_scalars32, const uint32_t* offsets, size_t n_msm,
                  uint8_t* out_blobs144, uint8_t* out_comp48) {
  return table_msm_host<FixedKind>(ctx, t, term_base, term_scalars32, offsets, n_msm, out_blobs144, out_comp48);
}
int cg1_fixed_msm_device(cg1_ctx* ctx, cg1_fixed* t, const void* d_term_base, const void* d_term_scalars32, const void* d_offsets, size_t n_msm,
                         size_t n_terms, size_t max_terms, void* d_out_affine96, void* d_out_comp48) {
  return table_msm_device<FixedKind>(ctx, t, d_term_base, d_term_scalars32, d_offsets, n_msm, n_terms, max_terms, d_out_affine96, d_out_comp48);
}
}  // extern "C"
