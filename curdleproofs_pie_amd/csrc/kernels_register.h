// Whisk REGISTRATIONS made in bulk: tracker (r_G | k_r_G), k_commitment k_G and opening proof (A | B | s) from the secret k -- the
// reference's generate_tracker (test_curdleproofs.py:759-790), get_k_commitment and GenerateWhiskTrackerProof
// (whisk_interface.py:177-190 -> opening.py:33-56) for many validators at once.  Part of the single translation unit csrc/msm_gpu.hip.
//
// The opening prover (kernels_opening.h) is handed a tracker and does not know r: it decodes r_G (a square root) and runs a 255-doubling
// ladder for B = b r_G.  The maker of a registration draws r itself, so all five points are multiples of the GENERATOR:
//     r_G = r G     k_r_G = (k r) G     k_G = k G     A = b G     B = (b r) G
// and come out of the context's table of G (kernels_generator.h: 32 mixed additions each, no doubling, no square root).
// cg1_whisk_register_device (capi_register.h) runs
//   k_register_scalars   status per item; r and b range-checked or drawn from the seed; the five canonical scalars in columns
//                        [k ... | b ... | r ... | k r ... | b r ...]  (the first two columns are the opening prover's gen_scalars)
//   k_register_points    the five multiples of one item on ONE lane with ONE inversion (Montgomery's trick over the five ZZ * ZZZ), encoded
//                        in columns [k_G ... | A ... | r_G ... | k_r_G ... | B ...] = the opening prover's gen48, wire and b48 back to back
//   k_prove_gather, cg1_merlin_batch_device (opening_transcript_program), k_prove_response    unchanged (kernels_opening.h)
//   k_register_trackers  the wire columns interleaved to n x (r_G | k_r_G); zeros for a refused item
#pragma once
#include "fr.h"

namespace cg1reg {
using cg1fr::fr;
using cg1open::Seed32;

// Draw d (0: r, 1: b) of the registration with global index `index`:
//   int.from_bytes(SHAKE256(b"whisk_registration_draw" || seed || le64(index) || le32(d)).digest(64), "little") mod r
// 67 input bytes fit one 136-byte rate block; blinder_from_seed's sponge layout (kernels_opening.h).  The host's copy is
// cg1_whisk_register_draws; registration.registration_draws_from_seed (hashlib) is the definition tests hold both to.
__device__ __forceinline__ fr draw_from_seed(uint32_t* sponge /* &lds[lane], stride LANES */, const Seed32& seed, uint32_t index, uint32_t d) {
  constexpr int L = cg1merlin::LANES;
  uint8_t msg[68];
  for (int k = 0; k < 68; ++k) msg[k] = 0;
  const char dom[] = "whisk_registration_draw";           // 23 bytes
  for (int k = 0; k < 23; ++k) msg[k] = (uint8_t)dom[k];
  for (int k = 0; k < 32; ++k) msg[23 + k] = (uint8_t)(seed.w[k >> 2] >> (8 * (k & 3)));
  for (int k = 0; k < 4; ++k) msg[55 + k] = (uint8_t)(index >> (8 * k));   // le64(index), index < 2^32
  for (int k = 0; k < 4; ++k) msg[63 + k] = (uint8_t)(d >> (8 * k));       // le32(d)
  msg[67] = 0x1Fu;                                        // SHAKE domain bits + first pad bit
  for (int k = 0; k < 50; ++k) sponge[k * L] = 0;
  for (int k = 0; k < 17; ++k)
    sponge[k * L] = (uint32_t)msg[4 * k] | ((uint32_t)msg[4 * k + 1] << 8) | ((uint32_t)msg[4 * k + 2] << 16) | ((uint32_t)msg[4 * k + 3] << 24);
  sponge[33 * L] = 0x80000000u;                           // last pad bit: byte 135 of the rate
  cg1merlin::keccak_words<false>(sponge);
  uint32_t o[16];
  for (int k = 0; k < 16; ++k) o[k] = sponge[k * L];
  return cg1fr::fr_from_le64_wide(reinterpret_cast<const uint8_t*>(o));
}

// status codes passed in (include/curdle_g1.h): k >= r; an r or b, supplied or drawn, that is zero or >= r.  rs and bs: both given or
// both null.  sc: five columns of n canonical little-endian scalars [k | b | r | k r | b r], zeros for a refused item.
__global__ void __launch_bounds__(64) k_register_scalars(const uint8_t* __restrict__ ks, const uint8_t* __restrict__ rs, const uint8_t* __restrict__ bs, Seed32 seed,
                                                         uint32_t first_index, uint32_t n, int32_t bad_scalar, int32_t bad_blinder, uint8_t* __restrict__ sc,
                                                         int32_t* __restrict__ status) {
  __shared__ uint32_t sponge[50 * cg1merlin::LANES];
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  fr k, r, b;
  int32_t st = 0;
  if (!cg1fr::fr_from_le32(ks + 32ull * i, k)) st = bad_scalar;
  else if (rs) {
    if (!cg1fr::fr_from_le32(rs + 32ull * i, r) || cg1fr::fr_is_zero(r) || !cg1fr::fr_from_le32(bs + 32ull * i, b) || cg1fr::fr_is_zero(b)) st = bad_blinder;
  } else {
    r = draw_from_seed(sponge + threadIdx.x, seed, first_index + i, 0u);
    b = draw_from_seed(sponge + threadIdx.x, seed, first_index + i, 1u);
    if (cg1fr::fr_is_zero(r) || cg1fr::fr_is_zero(b)) st = bad_blinder;
  }
  status[i] = st;
  uint8_t* col[5];
  for (int j = 0; j < 5; ++j) col[j] = sc + 32ull * ((size_t)j * n + i);
  if (st) {
    for (int j = 0; j < 5; ++j) for (int q = 0; q < 32; ++q) col[j][q] = 0;
    return;
  }
  cg1fr::fr_to_le32(k, col[0]);
  cg1fr::fr_to_le32(b, col[1]);
  cg1fr::fr_to_le32(r, col[2]);
  cg1fr::fr_to_le32(cg1fr::fr_mul(k, r), col[3]);
  cg1fr::fr_to_le32(cg1fr::fr_mul(b, r), col[4]);
}

// Five multiples of G per item, one lane per item, one inversion per item.
//
// The five sums run one after another through k_generator_mul's digit recoding and xyzz_madd (exceptional cases included), so one XYZZ
// accumulator is live at a time.  A finished sum leaves  D = ZZ ZZZ,  U = X ZZZ,  V = Y ZZ  and the running product of the D before it in
// the lane's own slot of `park` (x = U / D, y = V / D); after one fp_inv of the product of all D the lane reads its slot back, last sum
// first, and peels 1 / D_j off (Montgomery's trick).  An identity sum (k = 0 gives two) parks nothing, stays out of the product and is
// encoded 0xC0 00 .. 00.  Plain vector stores and loads of the lane's own words: no other lane reads them, no barrier.
//   park   REG_PARK_WORDS words per lane of the GRID, word q of lane t at park[q * lanes + t] (coalesced); a lane takes items t, t + lanes, ...
//   sc     5 columns of n canonical scalars (below r: the recoding's last carry is absorbed, kernels_generator.h)
//   enc    5 columns of n 48-byte encodings, column j = the multiples by column j of sc
constexpr int REG_POINTS = 5;
constexpr uint32_t REG_PARK_WORDS = REG_POINTS * 4 * cg1::NL;     // 280 words = 1 120 B per lane
constexpr uint32_t REG_MAX_BLOCKS = 512;                          // 256 CUs x 2 blocks of 256 lanes at the kernel's register count

__device__ __forceinline__ void park_store(uint32_t* __restrict__ slot, uint32_t lanes, int q, const cg1::fp& v) {
  for (int l = 0; l < cg1::NL; ++l) slot[(size_t)(q * cg1::NL + l) * lanes] = v.l[l];
}
__device__ __forceinline__ cg1::fp park_load(const uint32_t* __restrict__ slot, uint32_t lanes, int q) {
  cg1::fp v;
  for (int l = 0; l < cg1::NL; ++l) v.l[l] = slot[(size_t)(q * cg1::NL + l) * lanes];
  return v;
}

__global__ void __launch_bounds__(256) k_register_points(const cg1::PreparedPoint* __restrict__ tab, const uint32_t* __restrict__ sc, uint32_t n,
                                                         uint32_t* park, uint32_t* __restrict__ enc) {
  using namespace cg1;
  const uint32_t lanes = gridDim.x * 256, lane = blockIdx.x * 256 + threadIdx.x;
  uint32_t* slot = park + lane;
  for (uint32_t i = lane; i < n; i += lanes) {
    fp prod = fp_one();
    uint32_t live = 0;
#pragma unroll 1
    for (int j = 0; j < REG_POINTS; ++j) {
      const uint32_t* sw = sc + 8ull * ((size_t)j * n + i);
      uint64_t s[4];
      for (int k = 0; k < 4; ++k) s[k] = (uint64_t)sw[2 * k] | ((uint64_t)sw[2 * k + 1] << 32);
      const xyzz acc = generator_sum(tab, s);               // k_generator_mul's recoding and additions (kernels_generator.h)
      if (acc.inf) continue;
      live |= 1u << j;
      const fp D = fp_mul(acc.ZZ, acc.ZZZ);
      park_store(slot, lanes, 4 * j, prod);
      park_store(slot, lanes, 4 * j + 1, D);
      park_store(slot, lanes, 4 * j + 2, fp_mul(acc.X, acc.ZZZ));
      park_store(slot, lanes, 4 * j + 3, fp_mul(acc.Y, acc.ZZ));
      prod = fp_mul(prod, D);
    }
    fp inv = live ? fp_inv(prod) : prod;                    // 1 / (D_0 .. D_4) over the live sums
#pragma unroll 1
    for (int j = REG_POINTS - 1; j >= 0; --j) {
      const bool is_live = (live >> j) & 1u;
      uint32_t o[24];
      for (int k = 0; k < 24; ++k) o[k] = 0;
      if (is_live) {
        const fp t = fp_mul(inv, park_load(slot, lanes, 4 * j));          // 1 / D_j
        inv = fp_mul(inv, park_load(slot, lanes, 4 * j + 1));
        fp_to_words(fp_mul(park_load(slot, lanes, 4 * j + 2), t), o);
        fp_to_words(fp_mul(park_load(slot, lanes, 4 * j + 3), t), o + 12);
      }
      uint32_t c[12];
      compress_words(o, !is_live, c);
      uint32_t* dst = enc + 12ull * ((size_t)j * n + i);
      for (int k = 0; k < 12; ++k) dst[k] = c[k];
    }
  }
}

// wire = [r_G ...][k_r_G ...] -> trackers[i] = r_G | k_r_G; a refused item gets zeros
__global__ void __launch_bounds__(256) k_register_trackers(const uint32_t* __restrict__ wire, const int32_t* __restrict__ status, uint32_t n,
                                                           uint32_t* __restrict__ trackers) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 2u * n) return;
  const uint32_t i = t >> 1, j = t & 1u;
  const uint32_t* src = wire + 12ull * ((size_t)j * n + i);
  uint32_t* dst = trackers + 24ull * i + 12u * j;
  const bool ok = status[i] == 0;
  for (int k = 0; k < 12; ++k) dst[k] = ok ? src[k] : 0u;
}

}  // namespace cg1reg
