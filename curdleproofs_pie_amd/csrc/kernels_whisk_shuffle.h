// The device front of a Whisk shuffle proved from tracker bytes (capi_whisk_shuffle.h): what GenerateWhiskShuffleProof
// (whisk_interface.py:111-140) does between the pre-shuffle trackers and CurdleProofsProof.new -- decode, vec_T = perm(k vec_R),
// vec_U = perm(k vec_S), re-encode -- for every prover of a call at once.  The decoding and the subgroup test are the existing
// k_batch_decompress_row (kernels_batch.h) and k_subgroup_row (fp_row.h); the kernels here are
//     k_whisk_status        the call's status word: set when any of the call's points did not decode or lies outside G1
//     k_whisk_status_provers  the same per prover, with the first offending point: the seeded entry refuses shuffle by shuffle
//     k_whisk_permute_mul   out (p, h, i) = k_p * point perm[p][i] of half h of prover p, finished on the device: affine96 and the
//                           48-byte encoding, scattered into the tracker layout T_i | U_i
// and, for the seeded entry (cg1_whisk_shuffle_prove_seeded), the draws of every shuffle made on the device:
//     k_whisk_draws         one lane per (shuffle, draw): one SHAKE256 permutation -> a Fisher-Yates swap index or a scalar mod r
//     k_whisk_fisher_yates  the swaps of a shuffle applied in order -> its permutation
// Part of the single translation unit csrc/msm_gpu.hip (after kernels_fixed.h: row_inv, kernels_generator.h: compress_words, and
// kernels_opening.h: Seed32 and the sponge layout of blinder_from_seed).
#pragma once
#include "whisk_shuffle_host.h"

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

// status[p] = 0 for a clean prover, else code << 16 | (tracker 2 + half) of its FIRST offending point: a point the decoder refused
// (ST_NO_DECODE) before one outside G1 (ST_NOT_G1), each in tracker order -- the order whisk_front reports them in.  One block per prover.
constexpr uint32_t ST_NO_DECODE = 2u, ST_NOT_G1 = 3u;     // CG1_WHISK_SHUFFLE_NO_DECODE, CG1_WHISK_SHUFFLE_NOT_G1
__global__ void __launch_bounds__(64) k_whisk_status_provers(const uint8_t* __restrict__ decode_status, const uint8_t* __restrict__ in_g1, uint32_t ell,
                                                             uint32_t* __restrict__ status) {
  constexpr uint32_t NONE = 0xffffffffu;
  __shared__ uint32_t first[2];
  const uint32_t p = blockIdx.x, two = 2u * ell;
  if (threadIdx.x < 2u) first[threadIdx.x] = NONE;
  __syncthreads();
  uint32_t dec = NONE, g1 = NONE;
  for (uint32_t q = threadIdx.x; q < two; q += 64u) {      // q = tracker 2 + half, ascending within a lane
    const size_t at = (size_t)p * two + (size_t)(q & 1u) * ell + (q >> 1);
    if (dec == NONE && decode_status[at] != 0u) dec = q;
    if (g1 == NONE && in_g1[at] == 0u) g1 = q;
  }
  if (dec != NONE) atomicMin(&first[0], dec);
  if (g1 != NONE) atomicMin(&first[1], g1);
  __syncthreads();
  if (threadIdx.x == 0u) status[p] = first[0] != NONE ? (ST_NO_DECODE << 16 | first[0]) : first[1] != NONE ? (ST_NOT_G1 << 16 | first[1]) : 0u;
}

struct PermuteMulArgs {
  uint32_t ell, n_out;                       // n_out = P 2 ell
  const uint32_t* rs96;                      // [P][2][ell] affine96, standard form, zeros = the identity: vec_R | vec_S as decoded
  const uint32_t* perm;                      // [P][ell]
  const uint32_t* k;                         // [P] 8 words, little-endian, below r
  const uint32_t* status;                    // k_whisk_status's word
  const uint32_t* prover_status;             // nullable: k_whisk_status_provers' words; a prover whose word is set writes nothing
  uint32_t* tu96;                            // [P][2][ell] affine96: vec_T | vec_U
  uint32_t* post48;                          // [P][ell][2] 12 words each: T_i | U_i
};

// One WAVE per output point, as k_batch_mul_row: the scalar belongs to the wave, the window digit is wave-uniform, and the table of 15
// multiples stays in registers (a point is four VGPRs in row form).  The output is finished here -- one row_inv of ZZ ZZZ -- because
// nothing on the host wants the XYZZ form: the chain behind takes affine96, the caller takes the encoding.
// whisk_mul_finish: the wave's body, shared by k_whisk_permute_mul and k_chain_lineage_mul (kernels_chain_prove.h): scalar8 (8 words,
// little-endian, below r, wave-uniform) times the affine96 record at src96 (standard form, zeros = the identity) -> affine96 at d96 and
// the 48-byte encoding at d48 (ENC_ALWAYS; ENC_IF_NAMED: only where d48 is not null); lane 0 writes.  Registers, scratch and LDS of
// k_whisk_permute_mul are what they were with the body written out in the kernel: 188 VGPRs, 972 B scratch, no LDS.
constexpr int ENC_ALWAYS = 1, ENC_IF_NAMED = 2;
template <int ENC>
__device__ __forceinline__ void whisk_mul_finish(const uint32_t* src96, const uint32_t* scalar8, uint32_t* d96, uint32_t* d48) {
  const RowK k = row_constants();
  const uint32_t l = k.lane16;
  uint32_t r2 = 0;
#pragma unroll
  for (int t = 0; t < NL; ++t) r2 = l == (uint32_t)t ? fp_r2().l[t] : r2;
  xyzz_row P1;
  {
    const uint32_t* w = src96;
    uint32_t wd[24], any = 0;
    for (int t = 0; t < 24; ++t) { wd[t] = w[t]; any |= wd[t]; }
    P1.X = row_mul(row_from_fp(fp_from_words(wd), l), r2, k);
    P1.Y = row_mul(row_from_fp(fp_from_words(wd + 12), l), r2, k);
    P1.ZZ = k.one; P1.ZZZ = k.one; P1.inf = any ? 0u : 1u;
  }
  uint32_t s[8];
  for (int t = 0; t < 8; ++t) s[t] = scalar8[t];
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
  for (int t = 0; t < 24; ++t) d96[t] = w[t];
  if (ENC == ENC_ALWAYS || d48) {
    uint32_t c[12];
    compress_words(w, acc.inf != 0u, c);
    for (int t = 0; t < 12; ++t) d48[t] = c[t];
  }
}

__global__ void __launch_bounds__(64) k_whisk_permute_mul(PermuteMulArgs a) {
  const uint32_t o = blockIdx.x;
  if (o >= a.n_out || a.status[0] != 0u) return;           // (uniform) a refused call writes nothing
  const uint32_t ell = a.ell, two = 2u * ell;
  const uint32_t p = o / two, h = (o - p * two) / ell, i = o - p * two - h * ell;
  if (a.prover_status && a.prover_status[p] != 0u) return; // (uniform)
  uint32_t j = a.perm[(size_t)p * ell + i];
  j = j < ell ? j : ell - 1u;                              // the host has refused perm[i] >= ell; clamp all the same
  whisk_mul_finish<ENC_ALWAYS>(a.rs96 + 24ull * ((size_t)p * two + (size_t)h * ell + j), a.k + 8ull * p, a.tu96 + 24ull * o,
                         a.post48 + 12ull * (((size_t)p * ell + i) * 2u + h));
}

// ---- the seeded draws (the format: whisk_shuffle_host.h)
struct DrawArgs {
  cg1open::Seed32 seed;
  uint32_t ell, n_provers, first_index;      // first_index + n_provers <= 2^32: a shuffle's global index fits a word
  uint32_t* swaps;                           // [P][ell - 1]: j of the Fisher-Yates step i = ell - 1 - d, below i + 1
  uint32_t* scalars;                         // cg1whisk_host::DrawColumns, 8 words per scalar, canonical
};

// One lane per (shuffle, draw); the sponge of a lane sits in LDS at blinder_from_seed's stride.  D = ell + 3 n + 13 is no multiple of 64:
// the lanes of a wave belong to different shuffles and take either branch at the end.
__global__ void __launch_bounds__(cg1merlin::LANES) k_whisk_draws(DrawArgs a) {
  constexpr int L = cg1merlin::LANES;
  __shared__ uint32_t sponge[50 * L];
  const uint32_t D = cg1whisk_host::draw_count(a.ell);
  const uint32_t t = blockIdx.x * (uint32_t)L + threadIdx.x;               // P D <= 4096 * 3085
  if (t >= a.n_provers * D) return;
  const uint32_t p = t / D, d = t - p * D;
  uint8_t seedb[32], msg[64];
  for (int k = 0; k < 32; ++k) seedb[k] = (uint8_t)(a.seed.w[k >> 2] >> (8 * (k & 3)));
  cg1whisk_host::draw_message(seedb, a.first_index + p, d, msg);
  uint32_t* w = sponge + threadIdx.x;
  for (int k = 0; k < 50; ++k) w[k * L] = 0;
  for (int k = 0; k < 16; ++k)
    w[k * L] = (uint32_t)msg[4 * k] | ((uint32_t)msg[4 * k + 1] << 8) | ((uint32_t)msg[4 * k + 2] << 16) | ((uint32_t)msg[4 * k + 3] << 24);
  w[33 * L] = 0x80000000u;                                                 // last pad bit: byte 135 of the rate
  cg1merlin::keccak_words<false>(w);
  uint32_t o[16];
  for (int k = 0; k < 16; ++k) o[k] = w[k * L];
  if (d + 1u < a.ell) {
    const uint64_t lo = (uint64_t)o[0] | ((uint64_t)o[1] << 32), hi = (uint64_t)o[2] | ((uint64_t)o[3] << 32);
    a.swaps[(size_t)p * (a.ell - 1u) + d] = cg1whisk_host::draw_mod_u128(lo, hi, a.ell - d);
  } else {
    uint32_t v[8];
    cg1fr::fr_to_le32(cg1fr::fr_from_le64_wide(reinterpret_cast<const uint8_t*>(o)), reinterpret_cast<uint8_t*>(v));
    uint32_t* dst = a.scalars + 8u * cg1whisk_host::draw_slot(a.ell, a.n_provers, p, d - (a.ell - 1u));
    for (int k = 0; k < 8; ++k) dst[k] = v[k];
  }
}

// perm = list(range(ell)); for d = 0 .. ell - 2: i = ell - 1 - d, swap perm[i], perm[swaps[d]].  One block per shuffle: the row and its
// swaps come into LDS, ONE lane applies the swaps in order (each depends on the one before), all lanes write the row out.
__global__ void __launch_bounds__(64) k_whisk_fisher_yates(const uint32_t* __restrict__ swaps, uint32_t ell, uint32_t* __restrict__ perm) {
  __shared__ uint32_t pm[CG1_SAME_MSM_MAX_N], sw[CG1_SAME_MSM_MAX_N];
  const uint32_t p = blockIdx.x;
  if (ell > (uint32_t)CG1_SAME_MSM_MAX_N) return;          // (uniform; the host has refused it)
  for (uint32_t i = threadIdx.x; i < ell; i += 64u) {
    pm[i] = i;
    if (i + 1u < ell) sw[i] = swaps[(size_t)p * (ell - 1u) + i];
  }
  __syncthreads();
  if (threadIdx.x == 0u)
    for (uint32_t d = 0; d + 1u < ell; ++d) {
      const uint32_t i = ell - 1u - d, j = sw[d] <= i ? sw[d] : i;         // k_whisk_draws reduces below i + 1; clamp all the same
      const uint32_t x = pm[i];
      pm[i] = pm[j]; pm[j] = x;
    }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < ell; i += 64u) perm[(size_t)p * ell + i] = pm[i];
}

// ---- the witness kept on the device (the seeded entry with "whisk_resident_witness"): the draws' block -> the witness fields of a staging
// block, by the placement map of whisk_shuffle_host.h (PLACE_RULES resolved by the host into PlaceField, place_source called here).
// A copy and nothing else: blockIdx.y is the field, so the field's record is read once per wave from the kernel arguments and every
// branch on it is uniform; a lane moves 16 bytes.  The draws' columns and permutations begin on 64-byte boundaries, ChainLayout::take
// aligns the fields to 64, and ell is a multiple of 4 (ell + 4 a power of two >= 8), so every 16-byte piece is aligned on both sides; a
// row of words that is no multiple of 16 bytes would go a word per lane.  No LDS, no atomics; the stores are plain vector stores.
constexpr uint32_t PLACE_MAX_FIELDS = 8, PLACE_THREADS = 256;
struct PlaceArgs {
  const uint8_t* draws;                      // ctx->d_whisk_draws: DrawBlock
  uint8_t* block;                            // the table's staging block on the device
  uint32_t ell, Q, n_fields, pad;            // Q destination provers
  uint8_t keep[CG1_SAME_MSM_MAX_PROVERS];    // destination prover q reads prover keep[q] of the draws
  cg1whisk_host::PlaceField f[PLACE_MAX_FIELDS];
};
static_assert(CG1_SAME_MSM_MAX_PROVERS <= 256, "a prover's index fits a byte of PlaceArgs::keep");
__global__ void __launch_bounds__(PLACE_THREADS) k_whisk_witness_place(PlaceArgs a) {
  namespace W = cg1whisk_host;
  if (blockIdx.y >= a.n_fields) return;                    // (uniform)
  const W::PlaceField f = a.f[blockIdx.y];
  const uint32_t ell = a.ell, t = blockIdx.x * PLACE_THREADS + threadIdx.x;
  const bool words = f.kind == W::PLACE_WORDS;
  if (words && (f.dst_w & 3u) != 0u) {                     // (uniform) rows of words that are not 16-byte aligned: a word per lane
    if (t >= a.Q * f.dst_w) return;
    const uint32_t q = t / f.dst_w, e = t - q * f.dst_w;
    const W::PlaceSrc s = W::place_source(f, ell, a.keep[q], e);
    *reinterpret_cast<uint32_t*>(a.block + f.dst + 4ull * t) = *reinterpret_cast<const uint32_t*>(a.draws + s.at);
    return;
  }
  const uint32_t row16 = words ? f.dst_w / 4u : f.dst_w * 2u;              // 16-byte pieces of a destination row
  if (t >= a.Q * row16) return;
  const uint32_t q = t / row16, j = t - q * row16;
  const W::PlaceSrc s = W::place_source(f, ell, a.keep[q], words ? 4u * j : j >> 1);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (words) v = *reinterpret_cast<const uint4*>(a.draws + s.at);          // four entries of the row: they lie side by side in the source
  else if (s.bytes == 32u) v = *reinterpret_cast<const uint4*>(a.draws + s.at + 16u * (j & 1u));
  else if (s.bytes == 4u && (j & 1u) == 0u) v.x = *reinterpret_cast<const uint32_t*>(a.draws + s.at);       // a widened permutation entry
  *reinterpret_cast<uint4*>(a.block + f.dst + 16ull * t) = v;
}

}  // namespace cg1whisk
