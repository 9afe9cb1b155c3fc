// A chain of Whisk shuffles PROVED over the resident tracker set (capi_chain_prove.h; shuffle_chain.py: ShuffleChainProver,
// TrackerSet.evolve): every pre and post tracker of every block of a call in ONE launch without dependencies.  The host lineage
// (chain_lineage.h) has named, for every position, the ORIGIN slot of the set as it was before the call and the composite scalar (the product
// of the k's on the way, mod r); every origin a surviving block reads is certified in G1, where (k1 k2 mod r) P == k2 (k1 P).
//     k_chain_lineage_mul   out (b, w, half, t) = scalar[b][w][t] * point `half` of set slot origin[b][w][t]; w = 0: the pre records
//                           vec_R | vec_S of block b, w = 1: the post records vec_T | vec_U and their encodings T_t | U_t
// Part of the single translation unit csrc/msm_gpu.hip (after kernels_whisk_shuffle.h: whisk_mul_finish).
#pragma once

namespace cg1whisk {

struct LineageMulArgs {
  uint32_t ell, n_blocks, n_set_points;
  const uint32_t* set96;                     // the resident set: n_set_points affine96 records, r_G of slot s at 2 s, k_r_G at 2 s + 1
  const uint32_t* origin;                    // [n_blocks][2][ell] slot; 0xffffffff: a refused block, nothing is written for it
  const uint32_t* scalar;                    // [n_blocks][2][ell] 8 words, little-endian, below r
  uint32_t* rs96;                            // [n_blocks][2][ell] affine96: vec_R | vec_S
  uint32_t* tu96;                            // [n_blocks][2][ell] affine96: vec_T | vec_U
  uint32_t* post48;                          // [n_blocks][ell][2] 12 words each: T_t | U_t
};

// One WAVE per output point (whisk_mul_finish): the wave reads its origin's record from the set by index and its OWN scalar.  A pre
// position whose composite is 1 -- every first touch of a slot -- is the origin's record as it stands: a copy, the same bytes as the product.
__global__ void __launch_bounds__(64) k_chain_lineage_mul(LineageMulArgs a) {
  const uint32_t o = blockIdx.x, e = o >> 1, half = o & 1u;
  const uint32_t ell = a.ell, two = 2u * ell;
  if (e >= a.n_blocks * two) return;                       // (uniform, as every branch below)
  const uint32_t b = e / two, w = (e - b * two) / ell, t = e - b * two - w * ell;
  const uint32_t slot = a.origin[e];
  if (slot >= 0x7fffffffu || 2u * slot + half >= a.n_set_points) return;
  const uint32_t* src = a.set96 + 24ull * (2u * slot + half);
  const uint32_t* s = a.scalar + 8ull * e;
  const size_t at = (size_t)b * two + (size_t)half * ell + t;
  if (w == 0u) {
    uint32_t hi = 0;
    for (int i = 1; i < 8; ++i) hi |= s[i];
    if (s[0] == 1u && hi == 0u) {
      const uint32_t lane = threadIdx.x & 63u;
      if (lane < 24u) a.rs96[24ull * at + lane] = src[lane];
      return;
    }
  }
  whisk_mul_finish<ENC_IF_NAMED>(src, s, (w ? a.tu96 : a.rs96) + 24ull * at, w ? a.post48 + 12ull * (((size_t)b * ell + t) * 2u + half) : nullptr);
}

}  // namespace cg1whisk
