// C ABI, part 10: light tables of variable bases and the MSMs over them (kernels_light.h).
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

struct cg1_light : cg1_table {
  cg1::PointSum* d_tab = nullptr;                           // n_bases x LT_ENTRIES records (light_build)
};

namespace {
static_assert(CG1_LIGHT_MAX_MSMS <= CG1_FIXED_MAX_MSMS && CG1_LIGHT_MAX_TERMS <= CG1_FIXED_MAX_TERMS, "the light plan shares the fixed plan's ticket words, its LDS slices and k_fixed_finish");
struct LightKind {                                          // (FixedKind, capi_fixed.h)
  using Handle = cg1_light;
  using Plan = cg1::LightPlan;
  static constexpr const char* WHAT = "light-table MSM";
  static constexpr const char* ENTRY = "cg1_light_msm";
  static constexpr uint32_t MAX_MSMS = CG1_LIGHT_MAX_MSMS, MAX_TERMS = CG1_LIGHT_MAX_TERMS;
  static constexpr uint32_t FIRST_SLICE = 1, SLICE_8_WAVES = 2;
};

// The two launches of a table's build, enqueued on the context's stream: d_bases96 = n affine96 records on the device (curve points or
// all-zero records: the caller has checked), d_tab = room for n x LT_ENTRIES records.  Nothing waits here.
void light_build(cg1_ctx* ctx, const void* d_bases96, size_t n, cg1::PointSum* d_tab) {
  hipLaunchKernelGGL(cg1::k_light_chain, dim3((unsigned)n), dim3(64), 0, ctx->stream, (const uint32_t*)d_bases96, (uint32_t)n, d_tab);
  hipLaunchKernelGGL(cg1::k_light_multiples, dim3((unsigned)(n * cg1::LT_WINDOWS)), dim3(64), 0, ctx->stream, d_tab, (uint32_t)n);
}

// the device memory of a table of up to m bases and the words its MSM calls share; nothing is built
int light_alloc(cg1_ctx* ctx, cg1_light* t, size_t m) {
  HIPCHK(hipMalloc(&t->d_tab, m * (size_t)cg1::LT_ENTRIES * sizeof(cg1::PointSum)));
  return t->alloc(ctx);
}

// The light table a device prover builds inside its call over per-proof bases (capi_same_msm.h, capi_same_scalar.h): ONE scratch of
// records kept with the cg1_fixed handle the chain runs on, regrown only when a call needs more than it holds.  Nothing is built.
int chain_light_scratch(cg1_ctx* ctx, cg1_fixed* t, size_t m, cg1_light*& lt) {
  if (m > t->cap_smsm_bases) {
    if (t->smsm_light) cg1_light_destroy(t->smsm_light);
    t->smsm_light = new cg1_light();
    t->smsm_light->device = ctx->device;
    t->cap_smsm_bases = 0;
    { const int rc = light_alloc(ctx, t->smsm_light, m); if (rc) { cg1_light_destroy(t->smsm_light); t->smsm_light = nullptr; return rc; } }
    t->cap_smsm_bases = m;
  }
  lt = t->smsm_light;
  lt->n_bases = m;
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
  cg1::release_bufs({cg1::dev_buf(t->d_tab)});
  t->release();
  delete t;
}
size_t cg1_light_len(const cg1_light* t) { return t ? t->n_bases : 0; }
size_t cg1_light_bytes(const cg1_light* t) { return t ? t->n_bases * (size_t)cg1::LT_ENTRIES * sizeof(cg1::PointSum) : 0; }

int cg1_light_msm(cg1_ctx* ctx, cg1_light* t, const uint32_t* term_base, const uint8_t* term_scalars32, const uint32_t* offsets, size_t n_msm,
                  uint8_t* out_blobs144, uint8_t* out_comp48) {
  return table_msm_host<LightKind>(ctx, t, term_base, term_scalars32, offsets, n_msm, out_blobs144, out_comp48);
}
int cg1_light_msm_device(cg1_ctx* ctx, cg1_light* t, const void* d_term_base, const void* d_term_scalars32, const void* d_offsets, size_t n_msm,
                         size_t n_terms, size_t max_terms, void* d_out_affine96, void* d_out_comp48) {
  return table_msm_device<LightKind>(ctx, t, d_term_base, d_term_scalars32, d_offsets, n_msm, n_terms, max_terms, d_out_affine96, d_out_comp48);
}
}  // extern "C"
