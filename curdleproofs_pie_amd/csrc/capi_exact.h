// C ABI, part 20: exact relations in bulk on the device (kernels_exact.h).  The host twin cg1_exact_relations and the index check both
// entries share live beside the arithmetic they factor out of cg1_shuffle_exact_same_scalar (csrc/shuffle_verify.cpp).
// Part of the single translation unit csrc/msm_gpu.hip (included there; not a stand-alone header).
#pragma once

static_assert(CG1_EXACT_TERMS == cg1::EXACT_TERMS && CG1_EXACT_NEG == cg1::EXACT_NEG && CG1_EXACT_ONE == cg1::EXACT_ONE && CG1_EXACT_NONE == cg1::EXACT_NONE,
              "the record format of include/curdle_g1.h is the kernel's");

namespace {
// `bytes` of host records onto the device through one of the context's two page-locked staging blocks, taken in turn: *d_out is where the
// kernel launched next on the context's stream reads them.  The only wait is for the event behind the upload this block carried two calls ago.
int exact_stage(cg1_ctx* ctx, const void* host, size_t bytes, const void** d_out) {
  const int t = ctx->exact_turn;
  ctx->exact_turn ^= 1;
  if (!ctx->exact_ev[t]) HIPCHK(hipEventCreateWithFlags(&ctx->exact_ev[t], hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(ctx->exact_ev[t]));
  if (const int rc = cg1::grow_bufs(ctx, ctx->cap_exact[t], bytes, bytes, {cg1::host_buf(ctx->h_exact[t], bytes), cg1::dev_buf(ctx->d_exact[t], bytes)})) return rc;
  memcpy(ctx->h_exact[t], host, bytes);
  HIPCHK(hipMemcpyAsync(ctx->d_exact[t], ctx->h_exact[t], bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipEventRecord(ctx->exact_ev[t], ctx->stream));
  *d_out = ctx->d_exact[t];
  return CG1_OK;
}
}  // namespace

extern "C" {
int cg1_exact_relations_device(cg1_ctx* ctx, const void* d_points96, size_t n_points, const void* d_scalars32, size_t n_scalars,
                               const uint32_t* terms, size_t n_relations, void* d_ok) {
  if (!ctx) return CG1_ERR_HIP;
  if ((n_points && !d_points96) || (n_scalars && !d_scalars32) || (n_relations && !d_ok)) return CG1_ERR_ARG;
  // every index, on the host, before anything is copied or launched: the kernel reads nothing a record does not name
  if (const int rc = cg1_exact_relations_check(terms, n_relations, n_points, n_scalars)) {
    snprintf(ctx->err, sizeof ctx->err, "cg1_exact_relations_device: a record names a point or a scalar outside the arrays (%zu points, %zu scalars, %zu relations)",
             n_points, n_scalars, n_relations);
    return rc;
  }
  if (n_relations == 0) return CG1_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const void* d_terms = nullptr;
  if (const int rc = exact_stage(ctx, terms, n_relations * CG1_EXACT_TERMS * 8, &d_terms)) return rc;
  hipLaunchKernelGGL(cg1::k_exact_relations, dim3((unsigned)n_relations), dim3(64), 0, ctx->stream, (const uint32_t*)d_points96, (uint32_t)n_points,
                     (const uint32_t*)d_scalars32, (uint32_t)n_scalars, (const uint2*)d_terms, (uint32_t)n_relations, (uint8_t*)d_ok);
  HIPCHK(hipGetLastError());
  return CG1_OK;
}

int cg1_exact_gather_device(cg1_ctx* ctx, const void* d_src, size_t n_src_blocks, size_t src_stride_bytes, const uint32_t* idx, size_t n_idx,
                            void* d_dst, size_t dst_stride_bytes, size_t block_bytes, size_t clear_off, size_t clear_bytes) {
  if (!ctx) return CG1_ERR_HIP;
  if (n_idx == 0) return CG1_OK;
  if (!d_src || !d_dst || !idx || n_idx > 0xffffffffull || block_bytes == 0 || block_bytes > 0xffffffffull || ((src_stride_bytes | dst_stride_bytes | block_bytes | clear_off | clear_bytes) & 3) ||
      block_bytes > dst_stride_bytes || (src_stride_bytes && block_bytes > src_stride_bytes) || clear_off > block_bytes || clear_bytes > block_bytes - clear_off)
    return CG1_ERR_ARG;
  for (size_t j = 0; j < n_idx; ++j)
    if (idx[j] >= n_src_blocks) {
      snprintf(ctx->err, sizeof ctx->err, "cg1_exact_gather_device: index %zu names block %u of %zu", j, idx[j], n_src_blocks);
      return CG1_ERR_ARG;
    }
  HIPCHK(hipSetDevice(ctx->device));
  const void* d_idx = nullptr;
  if (const int rc = exact_stage(ctx, idx, n_idx * 4, &d_idx)) return rc;
  hipLaunchKernelGGL(cg1::k_exact_gather, dim3((unsigned)n_idx), dim3(256), 0, ctx->stream, (const uint32_t*)d_src, src_stride_bytes / 4, (const uint32_t*)d_idx,
                     (uint32_t)n_idx, (uint32_t*)d_dst, dst_stride_bytes / 4, (uint32_t)(block_bytes / 4), (uint32_t)(clear_off / 4), (uint32_t)((clear_off + clear_bytes) / 4));
  HIPCHK(hipGetLastError());
  return CG1_OK;
}
}  // extern "C"
