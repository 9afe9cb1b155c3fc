// The device front of a Whisk shuffle proved from tracker bytes (capi_whisk_shuffle.h): what GenerateWhiskShuffleProof
// (whisk_interface.py:111-140) does between the pre-shuffle trackers and CurdleProofsProof.new -- decode, vec_T = perm(k vec_R),
// vec_U = perm(k vec_S), re-encode -- for every prover of a call at once.  The decoding and the subgroup test are the existing
// k_batch_decompress_row (kernels_batch.h) and k_subgroup_row (fp_row.h); the kernels here are
//     k_whisk_status        the call's status word: set when any of the call's points did not decode or lies outside G1
//     k_whisk_permute_mul   out (p, h, i) = k_p * point perm[p][i] of half h of prover p, finished on the device: affine96 and the
//                           48-byte encoding, scattered into the tracker layout T_i | U_i
// Part of the single translation unit csrc/msm_gpu.hip (after kernels_fixed.h: row_inv, and kernels_generator.h: compress_words).
#pragma once

namespace cg1whisk {
using namespace cg1;

constexpr uint32_t ST_REFUSED = 1u;                       // the status word: some point of the call failed its decoding or the subgroup test

// status[0] |= ST_REFUSED when a decoding status is not CG1_OK or a subgroup flag is 0, over the n = P 2 ell points of the call.  The
// word is zero when the call begins (the host uploads it).
__global__ void __launch_bounds__(256) k_whisk_status(const uint8_t* __restrict__ decode_status, const uint8_t* __restrict__ in_g1, uint32_t n,
                                                      uint32_t* __restrict__ status) {
  uint32_t bad = 0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) bad |= (decode_status[i] != 0u || in_g1[i] == 0u) ? 1u : 0u;
  if (bad) atomicOr(status, ST_REFUSED);
}

struct PermuteMulArgs {
  uint32_t ell, n_out;                       // n_out = P 2 ell
  const uint32_t* rs96;                      // [P][2][ell] affine96, standard form, zeros = the identity: vec_R | vec_S as decoded
  const uint32_t* perm;                      // [P][ell]
  const uint32_t* k;                         // [P] 8 words, little-endian, below r
  const uint32_t* status;                    // k_whisk_status's word
  uint32_t* tu96;                            // [P][2][ell] affine96: vec_T | vec_U
  uint32_t* post48;                          // [P][ell][2] 12 words each: T_i | U_i
};

// One WAVE per output point, as k_batch_mul_row: k belongs to the prover and so to the wave, the window digit is wave-uniform, and the
// table of 15 multiples stays in registers (a point is four VGPRs in row form).  The output is finished here -- one row_inv of ZZ ZZZ --
// because nothing on the host wants the XYZZ form: the chain behind takes affine96, the caller takes the encoding.
__global__ void __launch_bounds__(64) k_whisk_permute_mul(PermuteMulArgs a) {
  const uint32_t o = blockIdx.x;
  if (o >= a.n_out || a.status[0] != 0u) return;           // (uniform) a refused call writes nothing
  const uint32_t ell = a.ell, two = 2u * ell;
  const uint32_t p = o / two, h = (o - p * two) / ell, i = o - p * two - h * ell;
  uint32_t j = a.perm[(size_t)p * ell + i];
  j = j < ell ? j : ell - 1u;                              // the host has refused perm[i] >= ell; clamp all the same
  const RowK k = row_constants();
  const uint32_t l = k.lane16;
  uint32_t r2 = 0;
#pragma unroll
  for (int t = 0; t < NL; ++t) r2 = l == (uint32_t)t ? fp_r2().l[t] : r2;
  xyzz_row P1;
  {
    const uint32_t* w = a.rs96 + 24ull * ((size_t)p * two + (size_t)h * ell + j);
    uint32_t wd[24], any = 0;
    for (int t = 0; t < 24; ++t) { wd[t] = w[t]; any |= wd[t]; }
    P1.X = row_mul(row_from_fp(fp_from_words(wd), l), r2, k);
    P1.Y = row_mul(row_from_fp(fp_from_words(wd + 12), l), r2, k);
    P1.ZZ = k.one; P1.ZZZ = k.one; P1.inf = any ? 0u : 1u;
  }
  uint32_t s[8];
  for (int t = 0; t < 8; ++t) s[t] = a.k[8ull * p + t];
  xyzz_row acc; acc.X = acc.Y = acc.ZZ = acc.ZZZ = 0; acc.inf = 1;
  if (!P1.inf) {
    xyzz_row T[15];                                                          // T[d - 1] = d P1
    T[0] = P1;
    T[1] = row_dbl(P1, k);
#pragma unroll
    for (int d = 2; d < 15; ++d) T[d] = (d & 1) ? row_dbl(T[(d - 1) / 2], k) : row_add(T[d - 1], P1, k);
#pragma unroll 1
    for (int nib = 63; nib >= 0; --nib) {
      acc = row_dbl(row_dbl(row_dbl(row_dbl(acc, k), k), k), k);
      const uint32_t d = (s[nib >> 3] >> ((nib & 7) * 4)) & 15u;            // wave-uniform
      if (d) {
        xyzz_row Td = T[0];
#pragma unroll
        for (int e = 1; e < 15; ++e) {
          const bool me = d == (uint32_t)(e + 1);
          Td.X = me ? T[e].X : Td.X; Td.Y = me ? T[e].Y : Td.Y; Td.ZZ = me ? T[e].ZZ : Td.ZZ; Td.ZZZ = me ? T[e].ZZZ : Td.ZZZ;
          Td.inf = me ? T[e].inf : Td.inf;                                  // (a multiple of a point of small order may be the identity)
        }
        acc = row_add(acc, Td, k);
      }
    }
  }
  // ---- the finish: x = X / ZZ = X ZZZ / (ZZ ZZZ), y = Y / ZZZ = Y ZZ / (ZZ ZZZ), every lane of the wave in the row products
  const uint32_t tinv = row_inv(row_mul(acc.ZZ, acc.ZZZ, k), k);
  const fp xf = fp_norm(row_to_fp(row_mul(acc.X, row_mul(tinv, acc.ZZZ, k), k)));
  const fp yf = fp_norm(row_to_fp(row_mul(acc.Y, row_mul(tinv, acc.ZZ, k), k)));
  if ((threadIdx.x & 63u) != 0u) return;                   // lane 0 leaves the Montgomery form, reduces and writes (k_fixed_finish's tail)
  uint32_t w[24];
  for (int t = 0; t < 24; ++t) w[t] = 0;
  if (!acc.inf) { fp_to_words(xf, w); fp_to_words(yf, w + 12); }
  uint32_t* d96 = a.tu96 + 24ull * o;
  for (int t = 0; t < 24; ++t) d96[t] = w[t];
  uint32_t c[12];
  compress_words(w, acc.inf != 0u, c);
  uint32_t* d48 = a.post48 + 12ull * (((size_t)p * ell + i) * 2u + h);
  for (int t = 0; t < 12; ++t) d48[t] = c[t];
}

}  // namespace cg1whisk
