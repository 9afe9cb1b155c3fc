// The refusals cg1_whisk_shuffle_front (capi_whisk_shuffle.h, on the device) and cg1_whisk_shuffle_front_emulate (lazy_host.cpp, its host
// twin for the CPU tests) share: one set of checks and one set of texts, so that the two cannot drift apart.  Host only, but for the few
// functions marked CG1WHISK_HD: the format of the seeded draws, which the device kernels (kernels_whisk_shuffle.h) and the host twin share.
// Also the column table of a shuffle's witness and the view over it (ShuffleWitness) that every host entry of the Whisk provers passes on.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "secret_wipe.h"
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

// ---- the seeded draws (cg1_whisk_shuffle_draws_device: k_whisk_draws, k_whisk_fisher_yates; cg1_whisk_shuffle_draws: lazy_host.cpp).
// Draw d of shuffle `index` is SHAKE256("whisk_shuffle_draw" || seed32 || le64(index) || le32(d)).digest(64): 62 bytes in, one permutation.
// d < ell - 1 are the Fisher-Yates swaps; scalar number s = d - (ell - 1) runs through k, vec_m_blinders (4), vec_a_blinders (2),
// vec_c_blinders (4), ipa_r (n), ipa_z_head (n - 2), r_t r_u r_a r_b r_k, vec_r (n), and lands in the COLUMN layout the chain takes:
// every column holds its P rows one after the other, the columns in that order.
#if defined(__HIPCC__)
#define CG1WHISK_HD __host__ __device__ inline
#else
#define CG1WHISK_HD inline
#endif
constexpr size_t DRAW_DOMAIN_LEN = 18;
constexpr char DRAW_DOMAIN[] = "whisk_shuffle_draw";
static_assert(sizeof DRAW_DOMAIN == DRAW_DOMAIN_LEN + 1, "");

CG1WHISK_HD uint32_t draw_scalars(uint32_t ell) { return 3u * (ell + (uint32_t)N_BLINDERS) + 14u; }        // per shuffle
CG1WHISK_HD uint32_t draw_count(uint32_t ell) { return ell - 1u + draw_scalars(ell); }                    // D = ell + 3 n + 13

// THE COLUMN TABLE: the eight scalar columns of a shuffle's witness in the order the draws fill them, and the scalars a prover's row of
// each holds (n = ell + 4).  Everything on the host that cuts, gathers or sizes a column reads the widths here.
enum Column { COL_K, COL_MBL, COL_ABL, COL_CBL, COL_IPA_R, COL_Z_HEAD, COL_BL, COL_VEC_R, N_COLUMNS };
inline size_t column_width(int column, size_t n) {
  const size_t width[N_COLUMNS] = {1, N_BLINDERS, 2, N_BLINDERS, n, n - 2, 5, n};
  return width[column];
}
// where the columns begin, in scalars, for P provers: k | vec_m_blinders | vec_a_blinders | vec_c_blinders | ipa_r | ipa_z_head | blinders | vec_r
struct DrawColumns { size_t at[N_COLUMNS], total; };
inline DrawColumns draw_columns(size_t ell, size_t P) {
  DrawColumns c;
  c.total = 0;
  for (int col = 0; col < N_COLUMNS; ++col) { c.at[col] = c.total; c.total += P * column_width(col, ell + N_BLINDERS); }
  return c;
}
// the slot (in scalars) of scalar number s of prover p: the same table spelt out for the device (it compiles into k_whisk_draws);
// tests/native/witness_gather.cpp holds the two against each other
CG1WHISK_HD size_t draw_slot(uint32_t ell, uint32_t P, uint32_t p, uint32_t s) {
  const size_t n = ell + (uint32_t)N_BLINDERS, Pz = P, pz = p;
  if (s < 1u) return pz;
  if (s < 5u) return Pz + 4 * pz + (s - 1u);
  if (s < 7u) return 5 * Pz + 2 * pz + (s - 5u);
  if (s < 11u) return 7 * Pz + 4 * pz + (s - 7u);
  if (s < 11u + n) return 11 * Pz + n * pz + (s - 11u);
  if (s < 9u + 2 * n) return (11 + n) * Pz + (n - 2) * pz + (s - 11u - n);
  if (s < 14u + 2 * n) return (9 + 2 * n) * Pz + 5 * pz + (s - 9u - 2 * n);
  return (14 + 2 * n) * Pz + n * pz + (s - 14u - 2 * n);
}
// (hi 2^64 + lo) mod m for 2 <= m <= 2^16: the swap index of a Fisher-Yates step from the first 16 bytes of its block
CG1WHISK_HD uint32_t draw_mod_u128(uint64_t lo, uint64_t hi, uint32_t m) {
  const uint64_t two64 = (~(uint64_t)0 % m + 1u) % m;
  return (uint32_t)(((hi % m) * two64 + lo % m) % m);
}
// the 64 message bytes of a draw's one rate block (the SHAKE domain byte included; the last pad bit, byte 135, is the caller's)
CG1WHISK_HD void draw_message(const uint8_t* seed32, uint32_t index, uint32_t d, uint8_t msg[64]) {
  for (int i = 0; i < 64; ++i) msg[i] = 0;
  for (size_t i = 0; i < DRAW_DOMAIN_LEN; ++i) msg[i] = (uint8_t)DRAW_DOMAIN[i];
  for (int i = 0; i < 32; ++i) msg[18 + i] = seed32[i];
  for (int i = 0; i < 4; ++i) { msg[50 + i] = (uint8_t)(index >> (8 * i)); msg[58 + i] = (uint8_t)(d >> (8 * i)); }      // le64(index), index < 2^32
  msg[62] = 0x1Fu;
}

// the refusals both draw entries share, after their pointer checks; nothing has been written when one is made.  The text (err: nullable)
// never holds the seed.
inline int check_draws(char* err, size_t err_len, const char* who, size_t ell, size_t P, uint64_t first_index) {
  if (!shape_ok(ell)) { if (err) snprintf(err, err_len, "%s: ell + %zu must be a power of two in 8 .. %d", who, N_BLINDERS, CG1_SAME_MSM_MAX_N); return CG1_ERR_ARG; }
  if (P > CG1_WHISK_SHUFFLE_DRAWS_MAX_PROVERS) {
    if (err) snprintf(err, err_len, "%s: more than %d shuffles in one call", who, CG1_WHISK_SHUFFLE_DRAWS_MAX_PROVERS);
    return CG1_ERR_ARG; }
  if (first_index > ((uint64_t)1 << 32) || first_index + P > ((uint64_t)1 << 32)) {
    if (err) snprintf(err, err_len, "%s: first_index + n_provers exceeds 2^32: a shuffle's index is below 2^32", who);
    return CG1_ERR_ARG; }
  return CG1_OK;
}

// M's scalar row: perm[i] as a 32-byte little-endian scalar, then the four blinders
inline void m_scalar_row(size_t ell, const uint32_t* perm, const uint8_t* vec_m_blinders32, uint8_t* out) {
  memset(out, 0, 32 * ell);
  for (size_t i = 0; i < ell; ++i) memcpy(out + 32 * i, perm + i, 4);
  memcpy(out + 32 * ell, vec_m_blinders32, 32 * N_BLINDERS);
}

// the draws' block on the device (ctx->d_whisk_draws): the Fisher-Yates swaps, the permutations, the scalars in the column layout, each on
// a 64-byte boundary; the host staging of a seeded entry holds [perm, total)
struct DrawBlock { size_t swaps, perm, scalars, total; };
inline DrawBlock draw_block(size_t ell, size_t P) {
  auto up = [](size_t b) { return (b + 63) & ~(size_t)63; };
  DrawBlock B;
  B.swaps = 0; B.perm = up(P * (ell - 1) * 4); B.scalars = B.perm + up(P * ell * 4);
  B.total = B.scalars + draw_columns(ell, P).total * 32;
  return B;
}

// ---- THE PLACEMENT MAP: which bytes of the draws' block land in which witness field of the two staging blocks a seeded call lays out --
// the front's (whisk_front: WhiskLayout) and the chain's (shuffle_prove: ShuffleLayout | SscalarLayout | GprodLayout | SmsmLayout).  The
// device kernel k_whisk_witness_place and the host emulation cg1_whisk_witness_block_emulate both read PLACE_RULES and call place_source;
// neither restates what goes where.  (The host staging of the copying path -- m_scalar_row, the *_stage functions -- is the OTHER
// statement of it, and tests/test_whisk_witness_place.py holds the two against each other byte for byte.)
enum PlaceKind : uint32_t {
  PLACE_WORDS,                               // 4-byte elements: a row of a permutation
  PLACE_SCALARS,                             // 32-byte elements: the first scalars of a column's row, zero scalars behind them
  PLACE_M_ROW                                // 32-byte elements: m_scalar_row -- perm[i] widened, ell times, then the four vec_m_blinders
};
enum PlaceBlock : uint8_t { BLOCK_FRONT, BLOCK_CHAIN };
// a field's phase: the launch that places it.  The chain's GprodLayout goes up at step 6 of shuffle_prove, behind the first host wait, so
// its fields are placed there (phase 1); everything else behind the uploads in front of the first kernel (phase 0)
enum PlaceFieldId { PF_L_PERM, PF_L_K, PF_MF_SC, PF_SH_PERM, PF_SH_ABL, PF_SS_K, PF_SS_BL, PF_GP_PERM, PF_GP_ABL, PF_GP_MBL, PF_GP_CBL, PF_GP_R, PF_GP_Z, PF_SM_VR,
                    N_PLACE_FIELDS };
struct PlaceRule { uint8_t block, phase; PlaceKind kind; int column; int dst_n, dst_c; };      // a prover's destination row: dst_n * n + dst_c elements (n = ell + 4)
constexpr PlaceRule PLACE_RULES[N_PLACE_FIELDS] = {
    {BLOCK_FRONT, 0, PLACE_WORDS, -1, 1, -4},              // L.perm
    {BLOCK_FRONT, 0, PLACE_SCALARS, COL_K, 0, 1},          // L.k
    {BLOCK_FRONT, 0, PLACE_M_ROW, COL_MBL, 1, 0},          // MF.sc
    {BLOCK_CHAIN, 0, PLACE_WORDS, -1, 1, -4},              // SH.perm
    {BLOCK_CHAIN, 0, PLACE_SCALARS, COL_ABL, 0, 2},        // SH.abl
    {BLOCK_CHAIN, 0, PLACE_SCALARS, COL_K, 0, 1},          // SS.k
    {BLOCK_CHAIN, 0, PLACE_SCALARS, COL_BL, 0, 5},         // SS.bl
    {BLOCK_CHAIN, 1, PLACE_WORDS, -1, 1, -4},              // GP.perm
    {BLOCK_CHAIN, 1, PLACE_SCALARS, COL_ABL, 0, 4},        // GP.abl: the two blinders, then two zero scalars
    {BLOCK_CHAIN, 1, PLACE_SCALARS, COL_MBL, 0, 4},        // GP.mbl
    {BLOCK_CHAIN, 1, PLACE_SCALARS, COL_CBL, 0, 4},        // GP.cbl
    {BLOCK_CHAIN, 1, PLACE_SCALARS, COL_IPA_R, 1, 0},      // GP.r
    {BLOCK_CHAIN, 1, PLACE_SCALARS, COL_Z_HEAD, 1, 0},     // GP.z: n - 2 scalars, then 64 zero bytes (the step kernel completes them)
    {BLOCK_CHAIN, 0, PLACE_SCALARS, COL_VEC_R, 1, 0},      // SM.vr
};
// a rule resolved for one call: byte offsets into the block and into the draws' block, row widths in elements
struct PlaceField {
  uint64_t dst;                              // of the field in the staging block
  uint64_t src, src2;                        // of row 0 of the source in the draws' block; PLACE_M_ROW: src the permutations, src2 vec_m_blinders
  uint32_t kind, dst_w, src_w, pad;          // src_w: the elements a source row holds (PLACE_M_ROW: its blinders)
};
inline PlaceField place_resolve(const PlaceRule& r, size_t ell, size_t P, size_t dst) {
  const size_t n = ell + N_BLINDERS;
  const DrawColumns C = draw_columns(ell, P);
  const DrawBlock B = draw_block(ell, P);
  const size_t perm_at = B.perm, scalars_at = B.scalars;
  PlaceField f{};
  f.dst = dst; f.kind = r.kind; f.dst_w = (uint32_t)(r.dst_n * (long)n + r.dst_c);
  if (r.kind == PLACE_WORDS) { f.src = perm_at; f.src_w = (uint32_t)ell; return f; }
  f.src = scalars_at + 32 * C.at[r.column]; f.src_w = (uint32_t)column_width(r.column, n);
  if (r.kind == PLACE_M_ROW) { f.src2 = f.src; f.src = perm_at; }
  return f;
}
// the bytes of a block's witness fields for P provers: the sum of the fields' lengths
inline size_t place_bytes(int block, size_t ell, size_t P) {
  const long n = (long)(ell + N_BLINDERS);
  size_t sum = 0;
  for (const PlaceRule& r : PLACE_RULES)
    if (r.block == block) sum += P * (size_t)(r.dst_n * n + r.dst_c) * (r.kind == PLACE_WORDS ? 4u : 32u);
  return sum;
}
CG1WHISK_HD uint32_t place_elem_bytes(const PlaceField& f) { return f.kind == PLACE_WORDS ? 4u : 32u; }
// THE FUNCTION: element e of destination prover q's row of field f comes from `bytes` bytes at `at` in the draws' block, the rest of the
// element zero (bytes == 0: a zero element); p = keep[q], the prover of the draws that destination prover q is
struct PlaceSrc { uint64_t at; uint32_t bytes; };
CG1WHISK_HD PlaceSrc place_source(const PlaceField& f, uint32_t ell, uint32_t p, uint32_t e) {
  PlaceSrc s; s.at = 0; s.bytes = 0;
  if (f.kind == PLACE_WORDS || (f.kind == PLACE_M_ROW && e < ell)) { s.at = f.src + 4ull * ((uint64_t)p * ell + e); s.bytes = 4u; return s; }
  if (f.kind == PLACE_M_ROW) { s.at = f.src2 + 32ull * ((uint64_t)p * f.src_w + (e - ell)); s.bytes = 32u; return s; }
  if (e < f.src_w) { s.at = f.src + 32ull * ((uint64_t)p * f.src_w + e); s.bytes = 32u; }
  return s;
}
// a field placed on the host: the emulation's loop over what the kernel does a lane per 16 bytes.  keep == NULL: q itself
inline void place_field_host(uint8_t* block, const PlaceField& f, const uint8_t* draws, size_t ell, const size_t* keep, size_t Q) {
  const size_t eb = place_elem_bytes(f);
  for (size_t q = 0; q < Q; ++q)
    for (size_t e = 0; e < f.dst_w; ++e) {
      const PlaceSrc s = place_source(f, (uint32_t)ell, (uint32_t)(keep ? keep[q] : q), (uint32_t)e);
      uint8_t* d = block + f.dst + (q * f.dst_w + e) * eb;
      memset(d, 0, eb);
      memcpy(d, draws + s.at, s.bytes);
    }
}

// The witness of P shuffles of one ell as the whole-shuffle prover takes it: the permutations (P rows of ell indices) and the eight scalar
// columns (P rows of column_width scalars each).  A view: it owns nothing, and whoever owns the bytes wipes them.
// Two variants.  HOST: perm and col point into host memory.  RESIDENT (d_draws set; perm and col null): the witness is the draws' block
// on the device, `draws_P` provers of it, of which this view's prover q is number keep[q] (keep == NULL: q) -- no byte of it is on the
// host, and whisk_front / shuffle_prove place it into their blocks with k_whisk_witness_place instead of staging it.
struct ShuffleWitness {
  size_t ell, P;
  const uint32_t* perm;
  const uint8_t* col[N_COLUMNS];
  const uint8_t* d_draws = nullptr;
  size_t draws_P = 0;
  const size_t* keep = nullptr;
  bool resident() const { return d_draws != nullptr; }
  static ShuffleWitness resident_draws(const uint8_t* d_draws, size_t ell, size_t P) {
    ShuffleWitness w{ell, P, nullptr, {}};
    w.d_draws = d_draws; w.draws_P = P;
    return w;
  }
  // the permutations at `perm`, the columns one after the other from `scalars`
  static ShuffleWitness over(const uint8_t* perm, const uint8_t* scalars, size_t ell, size_t P) {
    const DrawColumns C = draw_columns(ell, P);
    ShuffleWitness w{ell, P, reinterpret_cast<const uint32_t*>(perm), {}};
    for (int c = 0; c < N_COLUMNS; ++c) w.col[c] = scalars + 32 * C.at[c];
    return w;
  }
  // over the staging the draws of P shuffles come down into: [perm, total) of their DrawBlock
  static ShuffleWitness of_draws(const uint8_t* stage, size_t ell, size_t P) {
    const DrawBlock B = draw_block(ell, P);
    return over(stage, stage + (B.scalars - B.perm), ell, P);
  }
  // the rows keep[0] < keep[1] < .. < keep[Q - 1] of every column copied into `into`; all P rows: this view itself, and no copy
  // (a resident witness: the same view with the list as its index, and no copy -- `keep` must outlive it)
  ShuffleWitness gather(const size_t* keep, size_t Q, cg1::WipedBytes& into) const {
    if (resident()) { ShuffleWitness w = *this; w.P = Q; w.keep = keep; return w; }
    if (Q == P) return *this;
    into.v.assign(Q * ell * 4 + 32 * draw_columns(ell, Q).total, 0);
    uint8_t* base = into.v.data();
    const ShuffleWitness w = over(base, base + Q * ell * 4, ell, Q);
    for (size_t q = 0; q < Q; ++q) {
      memcpy(base + q * ell * 4, perm + keep[q] * ell, ell * 4);
      for (int c = 0; c < N_COLUMNS; ++c) {
        const size_t row = 32 * column_width(c, ell + N_BLINDERS);
        memcpy(base + (w.col[c] - base) + q * row, col[c] + keep[q] * row, row);
      }
    }
    return w;
  }
};

}  // namespace cg1whisk_host
