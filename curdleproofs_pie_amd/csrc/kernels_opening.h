// Whisk tracker-opening proofs (opening.py:21-79; IsValidWhiskOpeningProof, whisk_interface.py:147-169): the batch verifier's
// FRONT-END on the device -- what csrc/shuffle_verify.cpp cg1_opening_prepare does per proof on the host.  Part of the single
// translation unit csrc/msm_gpu.hip.
//
// The transcript of an opening proof is six 48-byte appends and one challenge (opening.py:60-71: k_G, G, k_r_G, r_G, A, B under
// "tracker_opening_proof", then "tracker_opening_proof_challenge"): four Keccak passes.  It runs through cg1_merlin_batch_device's
// block program on rows k_opening_gather lays out; the two kernels here are what surrounds it:
//   k_opening_gather    wire bytes -> the five own points per proof in MSM order [k_G, k_r_G, r_G, A, B] (what k_batch_decompress
//                       reads), and the transcript's data row [those five | G] -- any encoding with the infinity flag becomes the
//                       canonical 0xC0 00 .. 00 first, because the reference hashes points after RE-serialising them (util.py:27-32)
//   k_opening_scalars   challenge c, response s, weights rho1, rho2 -> the scalars of  rho1 (s G + c k_G - A) + rho2 (s r_G + c k_r_G - B)
//                       (opening.py:73-74 as one random combination), the proof's status, and zeros for a rejected proof
//   k_fr_sum            the generator's scalar: sum of rho1 s over the batch
#pragma once
#include "fr.h"

namespace cg1open {
using cg1fr::fr;

struct Enc48 { uint32_t w[12]; };
constexpr uint32_t ROW_BYTES = 288;                       // [k_G | k_r_G | r_G | A | B | G]

__global__ void __launch_bounds__(256) k_opening_gather(const uint32_t* __restrict__ trackers, const uint32_t* __restrict__ kcs, const uint32_t* __restrict__ proofs,
                                                        Enc48 g, uint32_t n, uint32_t* __restrict__ wire, uint32_t* __restrict__ rows) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 6u * n) return;
  const uint32_t i = t / 6u, j = t - 6u * i;
  uint32_t v[12];
  if (j == 5u) {
    for (int k = 0; k < 12; ++k) v[k] = g.w[k];
  } else {
    const uint32_t* src = j == 0u ? kcs + 12ull * i
                        : j == 1u ? trackers + 24ull * i + 12
                        : j == 2u ? trackers + 24ull * i
                        : j == 3u ? proofs + 32ull * i : proofs + 32ull * i + 12;
    for (int k = 0; k < 12; ++k) v[k] = src[k];
    if ((v[0] & 0xC0u) == 0xC0u) {                        // byte 0 of the encoding is the low byte of word 0
      v[0] = 0xC0u;
      for (int k = 1; k < 12; ++k) v[k] = 0;
    }
    uint32_t* w = wire + 12ull * (5ull * i + j);
    for (int k = 0; k < 12; ++k) w[k] = v[k];
  }
  uint32_t* r = rows + (size_t)(ROW_BYTES / 4) * i + 12u * j;
  for (int k = 0; k < 12; ++k) r[k] = v[k];
}

// The weights of a batch when the caller supplies none: rho1 | rho2 of proof i = the first 32 bytes of SHAKE256(seed || le64(i)), 128 bits
// each (a forger wins with probability 2^-128 per proof; the seed is 32 fresh bytes from the OS per batch and never leaves the verifier).
// Drawing 64 bytes per proof from the OS instead costs the host more than everything the GPU does for the proof.  The same function on
// the host: cg1_opening_weights_from_seed (shuffle_verify.cpp); tests compare both with hashlib.shake_256.
struct Seed32 { uint32_t w[8]; };
__device__ __forceinline__ void weights_from_seed(uint32_t* sponge /* &lds[lane], stride LANES */, const Seed32& seed, uint32_t i, uint8_t out64[64]) {
  constexpr int L = cg1merlin::LANES;
  for (int k = 0; k < 50; ++k) sponge[k * L] = 0;
  for (int k = 0; k < 8; ++k) sponge[k * L] = seed.w[k];
  sponge[8 * L] = i;                                       // le64(i), i < 2^32
  sponge[10 * L] = 0x1Fu;                                  // SHAKE domain bits + first pad bit at byte 40
  sponge[33 * L] = 0x80000000u;                            // last pad bit: byte 135 of the 136-byte rate
  cg1merlin::keccak_words<false>(sponge);
  uint32_t* o = reinterpret_cast<uint32_t*>(out64);
  for (int k = 0; k < 16; ++k) o[k] = 0;
  for (int k = 0; k < 4; ++k) { o[k] = sponge[k * L]; o[8 + k] = sponge[(4 + k) * L]; }
}

// status codes = csrc/shuffle_verify.cpp's (CG1_SHUFFLE_BAD_SCALAR / _BAD_WEIGHT / _BAD_POINT), passed in so that this file needs no header of it
__global__ void __launch_bounds__(64) k_opening_scalars(const uint8_t* __restrict__ challenges, const uint8_t* __restrict__ proofs, const uint8_t* __restrict__ weights,
                                                        Seed32 seed, const uint8_t* __restrict__ point_status, uint32_t n, int32_t bad_scalar, int32_t bad_weight, int32_t bad_point,
                                                        uint8_t* __restrict__ scalars, uint8_t* __restrict__ g_scalars, int32_t* __restrict__ status) {
  __shared__ uint32_t sponge[50 * cg1merlin::LANES];
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  alignas(8) uint8_t wbuf[64];
  const uint8_t* wt = wbuf;
  if (weights) wt = weights + 64ull * i;
  else weights_from_seed(sponge + threadIdx.x, seed, i, wbuf);
  uint64_t* sc = reinterpret_cast<uint64_t*>(scalars + 160ull * i);
  uint64_t* gs = reinterpret_cast<uint64_t*>(g_scalars + 32ull * i);
  fr s_, r1, r2, c;
  int32_t st = 0;
  if (!cg1fr::fr_from_le32(proofs + 128ull * i + 96, s_)) st = bad_scalar;
  else if (!cg1fr::fr_from_le32(wt, r1) || !cg1fr::fr_from_le32(wt + 32, r2)) st = bad_weight;
  else {
    const uint8_t* ps = point_status + 5ull * i;
    if (ps[0] | ps[1] | ps[2] | ps[3] | ps[4]) st = bad_point;
  }
  status[i] = st;
  if (st) {
    for (int k = 0; k < 20; ++k) sc[k] = 0;
    for (int k = 0; k < 4; ++k) gs[k] = 0;
    return;
  }
  cg1fr::fr_from_le32(challenges + 32ull * i, c);           // canonical by construction (curdleproofs_transcript.py:19-23)
  uint8_t* o = scalars + 160ull * i;
  cg1fr::fr_to_le32(cg1fr::fr_mul(r1, c), o);               // k_G
  cg1fr::fr_to_le32(cg1fr::fr_mul(r2, c), o + 32);          // k_r_G
  cg1fr::fr_to_le32(cg1fr::fr_mul(r2, s_), o + 64);         // r_G
  cg1fr::fr_to_le32(cg1fr::fr_neg(r1), o + 96);             // A
  cg1fr::fr_to_le32(cg1fr::fr_neg(r2), o + 128);            // B
  cg1fr::fr_to_le32(cg1fr::fr_mul(r1, s_), g_scalars + 32ull * i);      // G
}

// out[block] = sum of the block's slice of n canonical 32-byte scalars mod r (plain values add the same way as Montgomery ones); launched
// twice: gridDim.x partial sums, then one block over those
__global__ void __launch_bounds__(256) k_fr_sum(const uint64_t* __restrict__ v, uint32_t n, uint64_t* __restrict__ out) {
  __shared__ uint64_t sh[256][4];
  fr acc = cg1fr::fr_zero();
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += 256 * gridDim.x) acc = cg1fr::fr_add(acc, fr{{v[4ull * i], v[4ull * i + 1], v[4ull * i + 2], v[4ull * i + 3]}});
  for (int k = 0; k < 4; ++k) sh[threadIdx.x][k] = acc.l[k];
  __syncthreads();
  for (uint32_t d = 128; d >= 1; d >>= 1) {
    if (threadIdx.x < d) {
      const fr a{{sh[threadIdx.x][0], sh[threadIdx.x][1], sh[threadIdx.x][2], sh[threadIdx.x][3]}};
      const fr b{{sh[threadIdx.x + d][0], sh[threadIdx.x + d][1], sh[threadIdx.x + d][2], sh[threadIdx.x + d][3]}};
      const fr s = cg1fr::fr_add(a, b);
      for (int k = 0; k < 4; ++k) sh[threadIdx.x][k] = s.l[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) for (int k = 0; k < 4; ++k) out[4ull * blockIdx.x + k] = sh[0][k];
}

}  // namespace cg1open

// Whisk tracker-opening proofs, the PROVER's kernels (GenerateWhiskTrackerProof, whisk_interface.py:177-190 -> TrackerOpeningProof.new,
// opening.py:33-56): what csrc/shuffle_verify.cpp cg1_opening_prove does per proof on the host.  Part of the single translation unit
// csrc/msm_gpu.hip, next to the verifier's kernels above, whose row layout and transcript they share.
//
// Per proof, in the reference's order: decode k_r_G and r_G unchecked, k_G = k G, draw the blinder b, A = b G, B = b r_G, the six appends
// [k_G, G, k_r_G, r_G, A, B] and the challenge c, s = b - c k; the proof is A | B | s.  cg1_opening_prove_device runs
//   k_prove_split       n x (r_G | k_r_G) -> [r_G ...] [k_r_G ...]: the 2 n encodings k_batch_decompress reads, r_G's affine contiguous
//                       (the per-index bases of k_batch_mul)
//   k_batch_decompress  unchecked (util.py:35-36: a point outside G1 is legal and multiplied exactly)
//   k_prove_scalars     status per proof, blinders (given or seed-derived), the fixed-base scalars [k ... | b ...]
//   k_generator_mul     k_G, A compressed (kernels_generator.h);  k_batch_mul + k_batch_compress: B = b r_G
//   k_prove_gather      the transcript rows (k_opening_gather's layout), then cg1_merlin_batch_device: the challenges
//   k_prove_response    s = b - c k, the proof and k_G rows; zeros for a rejected proof
namespace cg1open {

__global__ void __launch_bounds__(256) k_prove_split(const uint32_t* __restrict__ trackers, uint32_t n, uint32_t* __restrict__ wire) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 2u * n) return;
  const uint32_t i = t >> 1, j = t & 1u;                  // j = 0: r_G, 1: k_r_G
  const uint32_t* src = trackers + 24ull * i + 12u * j;
  uint32_t* dst = wire + 12ull * ((size_t)j * n + i);
  for (int k = 0; k < 12; ++k) dst[k] = src[k];
}

// The blinder of proof i when the caller supplies none: int.from_bytes(SHAKE256(b"whisk_opening_blinder" || seed || le64(i)).digest(64),
// "little") mod r -- the first 64 bytes of one squeeze (61 input bytes fit one 136-byte rate block).  The host path derives the same
// blinders in Python (opening_prover.blinders_from_seed) and hands them to cg1_opening_prove; tests recompute them with hashlib.shake_256.
__device__ __forceinline__ cg1fr::fr blinder_from_seed(uint32_t* sponge /* &lds[lane], stride LANES */, const Seed32& seed, uint32_t i) {
  constexpr int L = cg1merlin::LANES;
  uint8_t msg[64];
  for (int k = 0; k < 64; ++k) msg[k] = 0;
  const char dom[] = "whisk_opening_blinder";             // 21 bytes
  for (int k = 0; k < 21; ++k) msg[k] = (uint8_t)dom[k];
  for (int k = 0; k < 32; ++k) msg[21 + k] = (uint8_t)(seed.w[k >> 2] >> (8 * (k & 3)));
  for (int k = 0; k < 4; ++k) msg[53 + k] = (uint8_t)(i >> (8 * k));   // le64(i), i < 2^32
  msg[61] = 0x1Fu;                                        // SHAKE domain bits + first pad bit
  for (int k = 0; k < 50; ++k) sponge[k * L] = 0;
  for (int k = 0; k < 16; ++k)
    sponge[k * L] = (uint32_t)msg[4 * k] | ((uint32_t)msg[4 * k + 1] << 8) | ((uint32_t)msg[4 * k + 2] << 16) | ((uint32_t)msg[4 * k + 3] << 24);
  sponge[33 * L] = 0x80000000u;                           // last pad bit: byte 135 of the rate
  cg1merlin::keccak_words<false>(sponge);
  uint32_t o[16];
  for (int k = 0; k < 16; ++k) o[k] = sponge[k * L];
  return cg1fr::fr_from_le64_wide(reinterpret_cast<const uint8_t*>(o));
}

// status codes passed in (csrc/shuffle_verify.cpp's): a tracker point that does not decode, k >= r, a blinder that is zero or >= r.
// gen_scalars: [k_0 .. k_{n-1} | b_0 .. b_{n-1}] (canonical, little-endian), zeros for a rejected proof.
__global__ void __launch_bounds__(64) k_prove_scalars(const uint8_t* __restrict__ point_status /* [r_G ...][k_r_G ...] */, const uint8_t* __restrict__ ks,
                                                      const uint8_t* __restrict__ blinders, Seed32 seed, uint32_t n, int32_t bad_point, int32_t bad_scalar,
                                                      int32_t bad_blinder, uint8_t* __restrict__ gen_scalars, int32_t* __restrict__ status) {
  __shared__ uint32_t sponge[50 * cg1merlin::LANES];
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  fr k, b;
  int32_t st = 0;
  if (point_status[n + i] | point_status[i]) st = bad_point;           // k_r_G, then r_G (whisk_interface.py:182-183): the same code either way
  else if (!cg1fr::fr_from_le32(ks + 32ull * i, k)) st = bad_scalar;
  else if (blinders) {
    if (!cg1fr::fr_from_le32(blinders + 32ull * i, b) || cg1fr::fr_is_zero(b)) st = bad_blinder;
  } else {
    b = blinder_from_seed(sponge + threadIdx.x, seed, i);
    if (cg1fr::fr_is_zero(b)) st = bad_blinder;
  }
  status[i] = st;
  uint8_t* gk = gen_scalars + 32ull * i;
  uint8_t* gb = gen_scalars + 32ull * ((size_t)n + i);
  if (st) {
    for (int q = 0; q < 32; ++q) { gk[q] = 0; gb[q] = 0; }
    return;
  }
  cg1fr::fr_to_le32(k, gk);
  cg1fr::fr_to_le32(b, gb);
}

// rows[i] = [k_G | k_r_G | r_G | A | B | G] (ROW_BYTES): gen48 = [k_G ...][A ...], b48 = [B ...], wire = [r_G ...][k_r_G ...] as sent.  The
// tracker's points enter the transcript RE-serialised (util.py:27-32): an encoding with the infinity flag becomes 0xC0 00 .. 00.
__global__ void __launch_bounds__(256) k_prove_gather(const uint32_t* __restrict__ gen48, const uint32_t* __restrict__ b48, const uint32_t* __restrict__ wire,
                                                      Enc48 g, uint32_t n, uint32_t* __restrict__ rows) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 6u * n) return;
  const uint32_t i = t / 6u, j = t - 6u * i;
  uint32_t v[12];
  if (j == 5u) {
    for (int k = 0; k < 12; ++k) v[k] = g.w[k];
  } else {
    const uint32_t* src = j == 0u ? gen48 + 12ull * i
                        : j == 1u ? wire + 12ull * ((size_t)n + i)
                        : j == 2u ? wire + 12ull * i
                        : j == 3u ? gen48 + 12ull * ((size_t)n + i) : b48 + 12ull * i;
    for (int k = 0; k < 12; ++k) v[k] = src[k];
    if ((v[0] & 0xC0u) == 0xC0u) {
      v[0] = 0xC0u;
      for (int k = 1; k < 12; ++k) v[k] = 0;
    }
  }
  uint32_t* r = rows + (size_t)(ROW_BYTES / 4) * i + 12u * j;
  for (int k = 0; k < 12; ++k) r[k] = v[k];
}

// s = b - c k (opening.py:52); proofs[i] = A | B | s, k_commitments[i] = k_G; a rejected proof gets zeros in both
__global__ void __launch_bounds__(256) k_prove_response(const uint8_t* __restrict__ challenges, const uint8_t* __restrict__ gen_scalars,
                                                        const uint32_t* __restrict__ gen48, const uint32_t* __restrict__ b48, const int32_t* __restrict__ status,
                                                        uint32_t n, uint32_t* __restrict__ proofs, uint32_t* __restrict__ k_commitments) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t* pf = proofs + 32ull * i;
  uint32_t* kc = k_commitments + 12ull * i;
  if (status[i]) {
    for (int q = 0; q < 32; ++q) pf[q] = 0;
    for (int q = 0; q < 12; ++q) kc[q] = 0;
    return;
  }
  fr c, k, b;
  cg1fr::fr_from_le32(challenges + 32ull * i, c);          // canonical by construction (curdleproofs_transcript.py:19-23)
  cg1fr::fr_from_le32(gen_scalars + 32ull * i, k);
  cg1fr::fr_from_le32(gen_scalars + 32ull * ((size_t)n + i), b);
  uint32_t s[8];
  cg1fr::fr_to_le32(cg1fr::fr_sub(b, cg1fr::fr_mul(c, k)), reinterpret_cast<uint8_t*>(s));
  const uint32_t* A = gen48 + 12ull * ((size_t)n + i);
  const uint32_t* B = b48 + 12ull * i;
  const uint32_t* kG = gen48 + 12ull * i;
  for (int q = 0; q < 12; ++q) { pf[q] = A[q]; pf[12 + q] = B[q]; kc[q] = kG[q]; }
  for (int q = 0; q < 8; ++q) pf[24 + q] = s[q];
}

}  // namespace cg1open
