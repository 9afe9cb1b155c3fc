// Fixed-base multiples of the generator G: out_i = k_i * G from a precomputed table, one lane per output.
// Part of the single translation unit csrc/msm_gpu.hip (included inside namespace cg1).
//
// k_batch_mul with nbase = 1 runs 255 doublings and ~128 mixed additions per output whatever the base; for the one base every
// Whisk opening proof multiplies twice (k_G = k G and A = b G, opening.py:33-56 / whisk_interface.py:186) the doublings can be
// paid once per context instead: signed c-bit digits of the scalar pick entries |d| * 2^(c w) * G of a table, and each output
// is ONE mixed addition per non-zero digit plus one inversion.  Window width c = 8: 32 windows x 128 entries (512 KiB of prepared
// records, gathered through L2), 32 mixed additions per output.  Measured against c = 4 (64 windows x 8 entries, 56 KiB staged in
// LDS per block, 64 additions): 9.7 against 13.5 ms for 2^20 outputs, k_batch_mul(nbase = 1) 63 ms
// (profiles/r06_opening_prover_window_ab.txt).
//
// Digits: a scalar is reduced below r first (k G == (k mod r) G), so it is < 2^255; recoded LSB first into d_w in
// [-2^(c-1), 2^(c-1)], the top window's value is at most 0x73 (r's top byte) before its carry, so the
// carry out of the last window is always absorbed: no extra window.  Every exceptional addition is exact (xyzz_madd:
// identity, equal and opposite operands).
constexpr int GEN_C = 8;                                  // window bits
constexpr int GEN_HALF = 1 << (GEN_C - 1);                // table entries per window: digits 1 .. 2^(c-1)
constexpr int GEN_WINDOWS = 256 / GEN_C;
constexpr int GEN_ENTRIES = GEN_WINDOWS * GEN_HALF;       // 4 096
static_assert(32 % GEN_C == 0, "a window never straddles two scalar words");

// affine std-form words (x[12] | y[12], little-endian) -> the 48-byte ZCash encoding as 12 words (byte 0 = low byte of word 0):
// k_batch_compress's rule (big-endian x, 0x80 compressed, 0x40 infinity, 0x20 "y > (p-1)/2")
__device__ __forceinline__ void compress_words(const uint32_t w[24], bool inf, uint32_t o[12]) {
  if (inf) {
    o[0] = 0xC0u;
    for (int k = 1; k < 12; ++k) o[k] = 0;
    return;
  }
  bool is_large = false, decided = false;
  for (int j = 11; j >= 0 && !decided; --j) if (w[12 + j] != W_P_MINUS_1_HALF[j]) { is_large = w[12 + j] > W_P_MINUS_1_HALF[j]; decided = true; }
  for (int j = 0; j < 12; ++j) o[j] = __builtin_bswap32(w[11 - j]);
  o[0] |= 0x80u | (is_large ? 0x20u : 0u);
}

// s * G for s below r (four little-endian 64-bit words): the recoding above and one mixed addition per non-zero digit.  Shared by
// k_generator_mul and k_register_points (kernels_register.h).
__device__ __forceinline__ xyzz generator_sum(const PreparedPoint* __restrict__ tab, const uint64_t s[4]) {
  xyzz acc = xyzz_identity();
  uint32_t carry = 0;
#pragma unroll 1
  for (int w = 0; w < GEN_WINDOWS; ++w) {
    const int bit = w * GEN_C;
    const uint32_t v = (uint32_t)(s[bit >> 6] >> (bit & 63)) & ((1u << GEN_C) - 1u);
    const uint32_t u = v + carry;
    carry = u > (uint32_t)GEN_HALF;
    const uint32_t mag = carry ? (1u << GEN_C) - u : u;   // |d|; d < 0 when carry
    if (!mag) continue;
    fp x, y;
    uint32_t fl;
    load_affine(tab + (w * GEN_HALF + (mag - 1)), x, y, fl);
    if (carry) y = fp_norm(fp_neg<3>(y));
    acc = xyzz_madd(acc, x, y);
  }
  return acc;
}

// tab: GEN_ENTRIES prepared records, entry w * GEN_HALF + (d - 1) = d * 2^(c w) * G.  scalars: n x 32 bytes little-endian, any value
// below 2^256.  out96 (affine std words, zeros = identity) and out48 (compressed) are each optional.
__global__ void __launch_bounds__(256) k_generator_mul(const PreparedPoint* __restrict__ tab, const uint32_t* __restrict__ scalars, uint32_t n,
                                                       uint32_t* __restrict__ out96, uint32_t* __restrict__ out48) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint64_t s[4];
  for (int k = 0; k < 4; ++k) s[k] = (uint64_t)scalars[8ull * i + 2 * k] | ((uint64_t)scalars[8ull * i + 2 * k + 1] << 32);
  for (int rep = 0; rep < 2; ++rep) {                     // 2^256 < 3 r: at most two subtractions
    bool ge = true;
    for (int k = 3; k >= 0; --k) if (s[k] != H_FR[k]) { ge = s[k] > H_FR[k]; break; }
    if (!ge) break;
    uint64_t borrow = 0;
    for (int k = 0; k < 4; ++k) {
      const uint64_t d = s[k] - H_FR[k] - borrow;
      borrow = (s[k] < H_FR[k] || (s[k] == H_FR[k] && borrow)) ? 1u : 0u;
      s[k] = d;
    }
  }
  const xyzz acc = generator_sum(tab, s);
  uint32_t o[24];
  for (int k = 0; k < 24; ++k) o[k] = 0;
  if (!acc.inf) {                                         // x = X/ZZ, y = Y/ZZZ with ONE inversion: 1/(ZZ*ZZZ)
    const fp t = fp_inv(fp_mul(acc.ZZ, acc.ZZZ));
    fp_to_words(fp_mul(acc.X, fp_mul(t, acc.ZZZ)), o);
    fp_to_words(fp_mul(acc.Y, fp_mul(t, acc.ZZ)), o + 12);
  }
  if (out96) {
    uint32_t* dst = out96 + 24ull * i;
    for (int k = 0; k < 24; ++k) dst[k] = o[k];
  }
  if (out48) {
    uint32_t c[12];
    compress_words(o, acc.inf, c);
    uint32_t* dst = out48 + 12ull * i;
    for (int k = 0; k < 12; ++k) dst[k] = c[k];
  }
}
