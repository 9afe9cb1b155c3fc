// C ABI, part 22: a chain of Whisk shuffles over a device-resident tracker set -- the strided decoding and the record moves around it
// (kernels_tracker_set.h).  The host half, cg1_chain_expand, lives in csrc/shuffle_verify.cpp.
// Part of the single translation unit csrc/msm_gpu.hip (included there, behind capi_exact.h whose staging blocks carry the index lists).
#pragma once

extern "C" {
// cg1_batch_decompress_enqueue (unchecked) through the index map (skip, take, stride): of every group of `stride` points the points
// [skip, skip + take) are decoded, the others are neither read nor written.  The three pointers name point 0 of group 0.
int cg1_batch_decompress_strided_enqueue(cg1_ctx* ctx, const void* d_in48, void* d_out_affine96, void* d_status, size_t n_groups, size_t stride,
                                         size_t skip, size_t take) {
  if (!ctx) return CG1_ERR_HIP;
  if (n_groups == 0 || take == 0) return CG1_OK;
  if (!d_in48 || !d_out_affine96 || !d_status || stride == 0 || skip > stride || take > stride - skip || n_groups >= (1ull << 31) / stride) return CG1_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t lanes = n_groups * take;
  const dim3 grid((unsigned)((lanes + 127) / 128)), block(128);
  if (ctx->decompress_waves == 3)
    hipLaunchKernelGGL((cg1::k_batch_decompress_strided<3>), grid, block, 0, ctx->stream, (const uint8_t*)d_in48, (uint32_t*)d_out_affine96, (uint8_t*)d_status,
                       (uint32_t)n_groups, (uint32_t)stride, (uint32_t)skip, (uint32_t)take);
  else
    hipLaunchKernelGGL((cg1::k_batch_decompress_strided<2>), grid, block, 0, ctx->stream, (const uint8_t*)d_in48, (uint32_t*)d_out_affine96, (uint8_t*)d_status,
                       (uint32_t)n_groups, (uint32_t)stride, (uint32_t)skip, (uint32_t)take);
  HIPCHK(hipGetLastError());
  return CG1_OK;
}

int cg1_chain_gather_enqueue(cg1_ctx* ctx, void* d_pts96, void* d_pstat, size_t n_points, const void* d_set_pts96, const void* d_set_pstat, size_t n_set_points,
                             const int32_t* plan, size_t first_group, size_t n_groups, size_t stride, size_t take) {
  if (!ctx) return CG1_ERR_HIP;
  if (n_groups == 0 || take == 0) return CG1_OK;
  if (!d_pts96 || !d_pstat || !plan || (n_set_points && (!d_set_pts96 || !d_set_pstat)) || (((uintptr_t)d_pts96 | (uintptr_t)d_set_pts96) & 15) || stride == 0 ||
      take > stride || n_points >= (1ull << 31) || n_set_points >= (1ull << 31) || first_group > n_points / stride || n_groups > n_points / stride - first_group || n_groups * take >= (1ull << 28))
    return CG1_ERR_ARG;
  // every entry, on the host, before anything is copied or launched: a source is a decoded position of an EARLIER group (never a gathered
  // one) or an entry of the set
  for (size_t g = 0; g < n_groups; ++g)
    for (size_t p = 0; p < take; ++p) {
      const int32_t s = plan[g * take + p];
      const bool good = s >= 0 ? ((size_t)s / stride < first_group + g && (size_t)s % stride >= take) : (size_t)(uint32_t)~s < n_set_points;
      if (!good) {
        snprintf(ctx->err, sizeof ctx->err, "cg1_chain_gather_enqueue: entry %zu of group %zu names %d (%zu set points, stride %zu, take %zu)", p, first_group + g, s,
                 n_set_points, stride, take);
        return CG1_ERR_ARG;
      }
    }
  HIPCHK(hipSetDevice(ctx->device));
  const void* d_plan = nullptr;
  if (const int rc = exact_stage(ctx, plan, n_groups * take * 4, &d_plan)) return rc;
  const size_t lanes = n_groups * take * 8;
  hipLaunchKernelGGL(cg1::k_chain_gather, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, (uint4*)d_pts96, (uint8_t*)d_pstat, (uint32_t)n_points,
                     (const uint4*)d_set_pts96, (const uint8_t*)d_set_pstat, (uint32_t)n_set_points, (const int32_t*)d_plan, (uint32_t)first_group, (uint32_t)n_groups,
                     (uint32_t)stride, (uint32_t)take);
  HIPCHK(hipGetLastError());
  return CG1_OK;
}

int cg1_chain_scatter_enqueue(cg1_ctx* ctx, const void* d_pts96, const void* d_pstat, size_t n_points, void* d_set_pts96, void* d_set_pstat, size_t n_set_points,
                              const uint32_t* pairs, size_t n_pairs) {
  if (!ctx) return CG1_ERR_HIP;
  if (n_pairs == 0) return CG1_OK;
  if (!d_pts96 || !d_pstat || !d_set_pts96 || !d_set_pstat || !pairs || (((uintptr_t)d_pts96 | (uintptr_t)d_set_pts96) & 15) || n_points >= (1ull << 31) ||
      n_set_points >= (1ull << 31) || n_pairs > n_set_points || n_pairs >= (1ull << 28))
    return CG1_ERR_ARG;
  std::vector<bool> seen(n_set_points, false);              // destinations are distinct: the launch has no write races
  for (size_t j = 0; j < n_pairs; ++j) {
    const uint32_t d = pairs[2 * j], s = pairs[2 * j + 1];
    if (d >= n_set_points || s >= n_points || seen[d]) {
      snprintf(ctx->err, sizeof ctx->err, "cg1_chain_scatter_enqueue: pair %zu (set point %u <- point %u) is out of range or repeats a set point", j, d, s);
      return CG1_ERR_ARG;
    }
    seen[d] = true;
  }
  HIPCHK(hipSetDevice(ctx->device));
  const void* d_pairs = nullptr;
  if (const int rc = exact_stage(ctx, pairs, n_pairs * 8, &d_pairs)) return rc;
  hipLaunchKernelGGL(cg1::k_chain_scatter, dim3((unsigned)((n_pairs * 8 + 255) / 256)), dim3(256), 0, ctx->stream, (const uint4*)d_pts96, (const uint8_t*)d_pstat,
                     (uint32_t)n_points, (uint4*)d_set_pts96, (uint8_t*)d_set_pstat, (uint32_t)n_set_points, (const uint2*)d_pairs, (uint32_t)n_pairs);
  HIPCHK(hipGetLastError());
  return CG1_OK;
}
}  // extern "C"
