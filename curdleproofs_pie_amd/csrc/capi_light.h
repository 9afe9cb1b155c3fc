// C ABI, part 10: light tables of variable bases and the MSMs over them (kernels_light.h).
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

struct cg1_light {
  int device = 0;
  size_t n_bases = 0;
  cg1::PointSum* d_tab = nullptr;                           // n_bases x LT_ENTRIES records (light_build)
  uint32_t* d_ctr = nullptr;                                // FX_MAX_MSMS + 8 words: tickets, finished MSMs, status bits; zero between calls
  uint32_t* d_status = nullptr;                             // 4 words: the status of a call that exports on the device only
  cg1::PointSum* d_partial = nullptr; size_t cap_partial = 0;
  cg1::PointSum* d_sum = nullptr;                           // FX_MAX_MSMS records for k_fixed_finish
  cg1::PointWords* h_out = nullptr; cg1::PointWords* h_out_dev = nullptr;      // pinned + mapped: FX_MAX_MSMS records + the status record
  uint8_t* h_in = nullptr; uint8_t* h_in_dev = nullptr; void* d_in = nullptr; size_t cap_in = 0;      // offsets | indices | scalars of a host call
};

namespace {
static_assert(CG1_LIGHT_MAX_MSMS <= CG1_FIXED_MAX_MSMS && CG1_LIGHT_MAX_TERMS <= CG1_FIXED_MAX_TERMS, "k_light_msm shares k_fixed_msm's ticket words, its LDS slices and k_fixed_finish");
// The two launches of a table's build, enqueued on the context's stream: d_bases96 = n affine96 records on the device (curve points or
// all-zero records: the caller has checked), d_tab = room for n x LT_ENTRIES records.  Nothing waits here.
void light_build(cg1_ctx* ctx, const void* d_bases96, size_t n, cg1::PointSum* d_tab) {
  hipLaunchKernelGGL(cg1::k_light_chain, dim3((unsigned)n), dim3(64), 0, ctx->stream, (const uint32_t*)d_bases96, (uint32_t)n, d_tab);
  hipLaunchKernelGGL(cg1::k_light_multiples, dim3((unsigned)(n * cg1::LT_WINDOWS)), dim3(64), 0, ctx->stream, d_tab, (uint32_t)n);
}

// the device memory of a table of up to m bases and the words its MSM calls share; nothing is built
int light_alloc(cg1_ctx* ctx, cg1_light* t, size_t m) {
  HIPCHK(hipMalloc(&t->d_tab, m * (size_t)cg1::LT_ENTRIES * sizeof(cg1::PointSum)));
  HIPCHK(hipMalloc(&t->d_ctr, (cg1::FX_MAX_MSMS + 8) * 4));
  HIPCHK(hipMalloc(&t->d_status, 16));
  HIPCHK(hipMalloc(&t->d_sum, (size_t)cg1::FX_MAX_MSMS * sizeof(cg1::PointSum)));
  HIPCHK(hipHostMalloc((void**)&t->h_out, ((size_t)cg1::FX_MAX_MSMS + 1) * sizeof(cg1::PointWords), hipHostMallocMapped | hipHostMallocCoherent));
  HIPCHK(hipHostGetDevicePointer((void**)&t->h_out_dev, t->h_out, 0));
  HIPCHK(hipMemsetAsync(t->d_ctr, 0, (cg1::FX_MAX_MSMS + 8) * 4, ctx->stream));
  HIPCHK(hipMemsetAsync(t->d_status, 0, 16, ctx->stream));
  return CG1_OK;
}

int light_create_impl(cg1_ctx* ctx, cg1_light* t, const uint8_t* bases96, size_t m) {
  for (size_t b = 0; b < m; ++b) {                          // canonical coordinates, on the curve (or the all-zero identity record)
    uint8_t blob[CG1_POINT_BYTES];
    const int rc = cg1_from_affine96(blob, bases96 + 96 * b, 1);
    if (rc != CG1_OK) { snprintf(ctx->err, sizeof ctx->err, "light-table base %zu: not a curve point (status %d)", b, rc); return rc; }
  }
  HIPCHK(hipSetDevice(ctx->device));
  DevBuf dbase;
  HIPCHK(dbase.alloc(m * 96));
  { const int rc = light_alloc(ctx, t, m); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(dbase.p, bases96, m * 96, hipMemcpyHostToDevice, ctx->stream));
  light_build(ctx, dbase.p, m, t->d_tab);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  return CG1_OK;
}

// fixed_pick_shape's rule (capi_fixed.h) for records a quarter as far apart: a term is up to LT_WINDOWS additions, twice k_fixed_msm's 32
// at c = 4, so the slices start at ONE term per workgroup -- the prover's shape, 4 MSMs of 64 terms, is then 256 workgroups of 8 waves,
// 8 dependent additions per wave and the tree.  "fixed_slice" / "fixed_waves" override here too.
template <typename F>
FixedShape light_pick_shape(const cg1_ctx* ctx, F groups, uint32_t M, uint32_t max_terms) {
  FixedShape sh{cg1::FX_MAX_SLICE, cg1::FX_WAVES};
  for (uint32_t s = 1; s < cg1::FX_MAX_SLICE; s <<= 1)
    if (groups(s) <= 256) { sh.slice = s; break; }
  if (sh.slice <= 2) sh.waves = 8;
  if (ctx->fixed_slice > 0 && (size_t)M * ((max_terms + ctx->fixed_slice - 1) / ctx->fixed_slice) <= 65536) sh.slice = (uint32_t)ctx->fixed_slice;
  if (ctx->fixed_waves > 0) sh.waves = (uint32_t)ctx->fixed_waves;
  return sh;
}

// enqueue k_light_msm (+ k_fixed_finish for device outputs); the term arrays are device-visible pointers
int light_enqueue(cg1_ctx* ctx, cg1_light* t, const uint32_t* d_tb, const uint32_t* d_sc, const uint32_t* d_offs, uint32_t M, uint32_t n_terms,
                  uint32_t max_terms, FixedShape shape, bool to_host, void* d_out96, void* d_out48) {
  const uint32_t slice = shape.slice;
  const uint32_t Smax = max_terms ? (max_terms + slice - 1) / slice : 1u;
  const size_t need = (size_t)M * Smax;
  if (Smax > 1 && need > t->cap_partial) {
    if (t->d_partial) (void)hipFree(t->d_partial);
    t->d_partial = nullptr; t->cap_partial = 0;
    HIPCHK(hipMalloc(&t->d_partial, need * sizeof(cg1::PointSum)));
    t->cap_partial = need;
  }
  cg1::LightArgs a;
  a.tab = t->d_tab; a.n_bases = (uint32_t)t->n_bases;
  a.term_base = d_tb; a.scalars = d_sc; a.offs = d_offs;
  a.M = M; a.n_terms = n_terms; a.max_terms = max_terms; a.slice = slice; a.Smax = Smax;
  a.partial = t->d_partial; a.counters = t->d_ctr;
  a.out_host = to_host ? t->h_out_dev : nullptr;
  a.status_out = to_host ? reinterpret_cast<uint32_t*>(t->h_out_dev + M) : t->d_status;
  a.flag_host = to_host ? ctx->h_flag_dev : nullptr;
  a.seq = to_host ? ++ctx->seq : 0u;
  a.out_sum = (d_out96 || d_out48) ? t->d_sum : nullptr;
  hipLaunchKernelGGL(cg1::k_light_msm, dim3(Smax, M), dim3(shape.waves * 64), 0, ctx->stream, a);
  if (a.out_sum)
    hipLaunchKernelGGL(cg1::k_fixed_finish, dim3((M + 3) / 4), dim3(64), 0, ctx->stream, (const cg1::PointSum*)t->d_sum, (const uint32_t*)a.status_out, M,
                       (uint32_t*)d_out96, (uint32_t*)d_out48);
  return CG1_OK;
}

int light_status_error(cg1_ctx* ctx, uint32_t st) {
  if (st & cg1::FX_BAD_OFFSETS) { snprintf(ctx->err, sizeof ctx->err, "light-table MSM: offsets not ascending, past the term arrays, or an MSM longer than max_terms"); return CG1_ERR_ARG; }
  if (st & cg1::FX_BAD_INDEX) { snprintf(ctx->err, sizeof ctx->err, "light-table MSM: a term's base index is outside the table"); return CG1_ERR_ARG; }
  if (st & cg1::FX_BAD_SCALAR) { snprintf(ctx->err, sizeof ctx->err, "light-table MSM: a scalar is >= r: scalar32 must be a canonical Fr element"); return CG1_ERR_ENCODING; }
  return CG1_OK;
}
}  // namespace

extern "C" {
cg1_light* cg1_light_create(cg1_ctx* ctx, const uint8_t* bases_affine96, size_t n_bases, int* status) {
  int rc = CG1_OK;
  cg1_light* t = nullptr;
  if (!ctx) rc = CG1_ERR_HIP;
  else if (!bases_affine96 || n_bases < 1 || n_bases > CG1_LIGHT_MAX_BASES) { snprintf(ctx->err, sizeof ctx->err, "a light table holds 1 .. %d bases", CG1_LIGHT_MAX_BASES); rc = CG1_ERR_ARG; }
  else {
    t = new cg1_light();
    t->device = ctx->device; t->n_bases = n_bases;
    rc = light_create_impl(ctx, t, bases_affine96, n_bases);
    if (rc != CG1_OK) { cg1_light_destroy(t); t = nullptr; }
  }
  if (status) *status = rc;
  return t;
}
void cg1_light_destroy(cg1_light* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  if (t->d_tab) (void)hipFree(t->d_tab);
  if (t->d_ctr) (void)hipFree(t->d_ctr);
  if (t->d_status) (void)hipFree(t->d_status);
  if (t->d_partial) (void)hipFree(t->d_partial);
  if (t->d_sum) (void)hipFree(t->d_sum);
  if (t->d_in) (void)hipFree(t->d_in);
  if (t->h_out) (void)hipHostFree(t->h_out);
  if (t->h_in) (void)hipHostFree(t->h_in);
  delete t;
}
size_t cg1_light_len(const cg1_light* t) { return t ? t->n_bases : 0; }
size_t cg1_light_bytes(const cg1_light* t) { return t ? t->n_bases * (size_t)cg1::LT_ENTRIES * sizeof(cg1::PointSum) : 0; }

int cg1_light_msm(cg1_ctx* ctx, cg1_light* t, const uint32_t* term_base, const uint8_t* term_scalars32, const uint32_t* offsets, size_t n_msm,
                  uint8_t* out_blobs144, uint8_t* out_comp48) {
  if (!ctx) return CG1_ERR_HIP;
  if (n_msm == 0) return CG1_OK;
  if (!t || !offsets || (!out_blobs144 && !out_comp48) || t->device != ctx->device) { snprintf(ctx->err, sizeof ctx->err, "cg1_light_msm: bad argument"); return CG1_ERR_ARG; }
  if (n_msm > CG1_LIGHT_MAX_MSMS) { snprintf(ctx->err, sizeof ctx->err, "cg1_light_msm: more than %d MSMs in one call", CG1_LIGHT_MAX_MSMS); return CG1_ERR_ARG; }
  const uint32_t M = (uint32_t)n_msm;
  uint32_t max_terms = 0;
  if (offsets[0] != 0) { snprintf(ctx->err, sizeof ctx->err, "cg1_light_msm: offsets[0] must be 0"); return CG1_ERR_ARG; }
  for (uint32_t j = 0; j < M; ++j) {
    if (offsets[j + 1] < offsets[j] || offsets[j + 1] - offsets[j] > CG1_LIGHT_MAX_TERMS) {
      snprintf(ctx->err, sizeof ctx->err, "cg1_light_msm: MSM %u: offsets not ascending or more than %d terms", j, CG1_LIGHT_MAX_TERMS);
      return CG1_ERR_ARG;
    }
    max_terms = std::max(max_terms, offsets[j + 1] - offsets[j]);
  }
  const uint32_t n = offsets[M];
  if (n && (!term_base || !term_scalars32)) { snprintf(ctx->err, sizeof ctx->err, "cg1_light_msm: bad argument"); return CG1_ERR_ARG; }
  for (uint32_t i = 0; i < n; ++i) {                        // the whole call is refused before anything is written
    if ((term_base[i] & 0x7fffffffu) >= t->n_bases) return light_status_error(ctx, cg1::FX_BAD_INDEX);
    uint32_t s[8];
    memcpy(s, term_scalars32 + 32 * (size_t)i, 32);
    if (!cg1::fixed_scalar_below_r(s)) return light_status_error(ctx, cg1::FX_BAD_SCALAR);
  }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->pend.active = false;
  // one page-locked block: offsets | indices | scalars
  const size_t o_tb = ((size_t)(M + 1) * 4 + 15) & ~(size_t)15, o_sc = (o_tb + (size_t)n * 4 + 15) & ~(size_t)15, bytes = o_sc + (size_t)n * 32;
  if (bytes > t->cap_in) {
    if (t->h_in) (void)hipHostFree(t->h_in);
    if (t->d_in) (void)hipFree(t->d_in);
    t->h_in = nullptr; t->d_in = nullptr; t->cap_in = 0;
    const size_t cap = std::max<size_t>(bytes + bytes / 4, 64 * 1024);
    HIPCHK(hipHostMalloc((void**)&t->h_in, cap, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer((void**)&t->h_in_dev, t->h_in, 0));
    HIPCHK(hipMalloc(&t->d_in, cap));
    t->cap_in = cap;
  }
  memcpy(t->h_in, offsets, (size_t)(M + 1) * 4);
  if (n) { memcpy(t->h_in + o_tb, term_base, (size_t)n * 4); memcpy(t->h_in + o_sc, term_scalars32, (size_t)n * 32); }
  const uint8_t* src = t->h_in_dev;
  if (bytes > FX_ZERO_COPY_MAX) {
    HIPCHK(hipMemcpyAsync(t->d_in, t->h_in, bytes, hipMemcpyHostToDevice, ctx->stream));
    src = static_cast<const uint8_t*>(t->d_in);
  }
  const FixedShape shape = light_pick_shape(ctx, [&](uint32_t s) { size_t g = 0; for (uint32_t j = 0; j < M; ++j) g += std::max<uint32_t>(1u, (offsets[j + 1] - offsets[j] + s - 1) / s); return g; }, M, max_terms);
  { const int rc = light_enqueue(ctx, t, (const uint32_t*)(src + o_tb), (const uint32_t*)(src + o_sc), (const uint32_t*)src, M, n, max_terms, shape, true, nullptr, nullptr); if (rc) return rc; }
  const uint32_t seq = ctx->seq;
  if (!ctx->blocking_sync) {
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
  } else {
    int wrc = cg1::wait_stream(ctx); if (wrc) return wrc;
  }
  HIPCHK(hipGetLastError());
  { const int rc = light_status_error(ctx, reinterpret_cast<const uint32_t*>(t->h_out + M)[0]); if (rc) return rc; }
  std::vector<uint8_t> tmp;
  uint8_t* blobs = out_blobs144;
  if (!blobs) { tmp.resize((size_t)M * CG1_POINT_BYTES); blobs = tmp.data(); }
  for (uint32_t j = 0; j < M; ++j) blob_out(blobs + (size_t)CG1_POINT_BYTES * j, cg1::jac_from_words(t->h_out[j]));
  if (out_comp48) cg1_batch_compress(out_comp48, blobs, M);
  return CG1_OK;
}

int cg1_light_msm_device(cg1_ctx* ctx, cg1_light* t, const void* d_term_base, const void* d_term_scalars32, const void* d_offsets, size_t n_msm,
                         size_t n_terms, size_t max_terms, void* d_out_affine96, void* d_out_comp48) {
  if (!ctx) return CG1_ERR_HIP;
  if (n_msm == 0) return CG1_OK;
  if (!t || !d_offsets || (!d_out_affine96 && !d_out_comp48) || t->device != ctx->device || (n_terms && (!d_term_base || !d_term_scalars32)) ||
      n_msm > CG1_LIGHT_MAX_MSMS || max_terms > CG1_LIGHT_MAX_TERMS || max_terms > n_terms || n_terms > (size_t)CG1_LIGHT_MAX_MSMS * CG1_LIGHT_MAX_TERMS) {
    snprintf(ctx->err, sizeof ctx->err, "cg1_light_msm_device: bad argument");
    return CG1_ERR_ARG;
  }
  HIPCHK(hipSetDevice(ctx->device));
  ctx->pend.active = false;
  const uint32_t M = (uint32_t)n_msm, mt = (uint32_t)max_terms;
  const FixedShape shape = light_pick_shape(ctx, [&](uint32_t s) { return (size_t)M * std::max<uint32_t>(1u, (mt + s - 1) / s); }, M, mt);
  { const int rc = light_enqueue(ctx, t, (const uint32_t*)d_term_base, (const uint32_t*)d_term_scalars32, (const uint32_t*)d_offsets, M, (uint32_t)n_terms, mt, shape, false,
                                 d_out_affine96, d_out_comp48); if (rc) return rc; }
  uint32_t st[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(st, t->d_status, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  return light_status_error(ctx, st[0]);
}
}  // extern "C"
