// The refusals cg1_whisk_shuffle_front (capi_whisk_shuffle.h, on the device) and cg1_whisk_shuffle_front_emulate (lazy_host.cpp, its host
// twin for the CPU tests) share: one set of checks and one set of texts, so that the two cannot drift apart.  Host only.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../include/curdle_g1.h"

namespace cg1whisk_host {

constexpr size_t N_BLINDERS = 4;

inline bool scalar_below_r(const uint8_t* le32) {
  static const uint64_t R[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
  uint64_t w[4];
  memcpy(w, le32, 32);
  for (int i = 3; i >= 0; --i)
    if (w[i] != R[i]) return w[i] < R[i];
  return false;
}

// ell + 4 a power of two in 8 .. CG1_SAME_MSM_MAX_N
inline bool shape_ok(size_t ell) {
  const size_t n = ell + N_BLINDERS;
  return ell >= 1 && n > ell && n >= 8 && (n & (n - 1)) == 0 && n <= CG1_SAME_MSM_MAX_N;
}

inline int check_shape(char* err, size_t err_len, const char* who, size_t ell) {
  if (shape_ok(ell)) return CG1_OK;
  snprintf(err, err_len, "%s: ell + %zu must be a power of two in 8 .. %d", who, N_BLINDERS, CG1_SAME_MSM_MAX_N);
  return CG1_ERR_ARG;
}

// the refusals that need no point arithmetic, in the order both entries make them (after their pointer and shape checks)
inline int check_inputs(char* err, size_t err_len, const char* who, size_t ell, size_t P, const uint32_t* perm, const uint8_t* k32, const uint8_t* vec_m_blinders32) {
  for (size_t p = 0; p < P; ++p)
    for (size_t i = 0; i < ell; ++i)
      if (perm[p * ell + i] >= ell) { snprintf(err, err_len, "%s: prover %zu: permutation entry %zu is %u, not below ell = %zu", who, p, i, perm[p * ell + i], ell); return CG1_ERR_ARG; }
  for (size_t p = 0; p < P; ++p) {
    if (!scalar_below_r(k32 + 32 * p)) { snprintf(err, err_len, "%s: prover %zu: k is >= r: scalar32 must be a canonical Fr element", who, p); return CG1_ERR_ENCODING; }
    for (size_t b = 0; b < N_BLINDERS; ++b)
      if (!scalar_below_r(vec_m_blinders32 + 32 * (p * N_BLINDERS + b))) {
        snprintf(err, err_len, "%s: prover %zu: vec_m_blinders[%zu] is >= r: scalar32 must be a canonical Fr element", who, p, b);
        return CG1_ERR_ENCODING;
      }
  }
  return CG1_OK;
}

// a tracker point the call refuses: rc is the decoder's status or CG1_ERR_NOT_IN_SUBGROUP; half 0 = r_G, 1 = k_r_G
inline int refuse_point(char* err, size_t err_len, const char* who, size_t prover, size_t index, int half, int rc) {
  const char* what = rc == CG1_ERR_ENCODING ? "is not a compressed encoding with x < p" : rc == CG1_ERR_NOT_ON_CURVE ? "is not on the curve"
                   : "lies outside the prime-order subgroup G1 (k folds into the scalars only for points of order r)";
  snprintf(err, err_len, "%s: prover %zu: tracker %zu: %s %s", who, prover, index, half ? "k_r_G" : "r_G", what);
  return rc;
}

// M's scalar row: perm[i] as a 32-byte little-endian scalar, then the four blinders
inline void m_scalar_row(size_t ell, const uint32_t* perm, const uint8_t* vec_m_blinders32, uint8_t* out) {
  memset(out, 0, 32 * ell);
  for (size_t i = 0; i < ell; ++i) memcpy(out + 32 * i, perm + i, 4);
  memcpy(out + 32 * ell, vec_m_blinders32, 32 * N_BLINDERS);
}

}  // namespace cg1whisk_host
