// A chain of Whisk shuffles over a tracker set that stays on the device in decoded form (shuffle_chain.py): the record moves around the
// strided decoding (k_batch_decompress_strided, kernels_batch.h).
// Part of the single translation unit csrc/msm_gpu.hip (included inside namespace cg1).
//
// A record is a decoded point: 96 bytes of affine standard-form words (zeros = the identity or a refused encoding) and the decoder's status
// byte.  Two arrays hold records: the batch's own points (`pts` / `pstat`, n proofs x L points) and the resident set (2 points per tracker:
// r_G at 2 s, k_r_G at 2 s + 1).
//   k_chain_gather   every pre position of the proofs of a sub-batch <- its source: an earlier proof's post position of the same batch
//                    (plan entry >= 0: a point index of `pts`) or an entry of the set (plan entry < 0: ~(set point index))
//   k_chain_scatter  set point pairs[2 j] <- batch point pairs[2 j + 1]: the final post of every slot a batch wrote
// Eight lanes per record: lanes 0..5 move 16 bytes each, lane 6 the status byte.  A source is a position the decoder wrote, never a gathered
// one, and the destinations of one launch are distinct, so a launch has no dependencies inside.  Every index has been checked on the host
// (capi_tracker_set.h); an entry out of range here is skipped.
#pragma once

// (no __restrict__: the gather reads and writes the same arrays, at different records)
__device__ __forceinline__ void chain_move_record(const uint4* src_pts, const uint8_t* src_stat, uint32_t src, uint4* dst_pts, uint8_t* dst_stat, uint32_t dst,
                                                  uint32_t lane8) {
  if (lane8 < 6u) dst_pts[6ull * dst + lane8] = src_pts[6ull * src + lane8];
  else if (lane8 == 6u) dst_stat[dst] = src_stat[src];
}

// plan: n_groups x take entries, entry e = g * take + p names the source of point (first_group + g) * stride + p
__global__ void __launch_bounds__(256) k_chain_gather(uint4* pts, uint8_t* pstat, uint32_t n_points,
                                                      const uint4* __restrict__ set_pts, const uint8_t* __restrict__ set_pstat, uint32_t n_set_points,
                                                      const int32_t* __restrict__ plan, uint32_t first_group, uint32_t n_groups, uint32_t stride, uint32_t take) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x, e = t >> 3, g = e / take;
  if (g >= n_groups) return;
  const uint32_t dst = (first_group + g) * stride + (e - g * take);
  const int32_t s = plan[e];
  if (dst >= n_points) return;
  if (s >= 0) {
    if ((uint32_t)s < n_points) chain_move_record(pts, pstat, (uint32_t)s, pts, pstat, dst, t & 7u);
  } else if ((uint32_t)~s < n_set_points) {
    chain_move_record(set_pts, set_pstat, (uint32_t)~s, pts, pstat, dst, t & 7u);
  }
}

__global__ void __launch_bounds__(256) k_chain_scatter(const uint4* __restrict__ pts, const uint8_t* __restrict__ pstat, uint32_t n_points,
                                                       uint4* __restrict__ set_pts, uint8_t* __restrict__ set_pstat, uint32_t n_set_points,
                                                       const uint2* __restrict__ pairs, uint32_t n_pairs) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x, j = t >> 3;
  if (j >= n_pairs) return;
  const uint2 p = pairs[j];                                  // x: set point, y: batch point
  if (p.x < n_set_points && p.y < n_points) chain_move_record(pts, pstat, p.y, set_pts, set_pstat, p.x, t & 7u);
}
