// Host half of the deferred-evaluation G1Point: see lazy_host.h.
#include "lazy_host.h"
#include "bls_consts.h"
#include "pool.h"
#include "ipa_rounds.h"
#include "same_msm_rounds.h"
#include "gprod_rounds.h"
#include "same_perm_rounds.h"
#include "same_scalar_rounds.h"
#include "shuffle_rounds.h"
#include "whisk_shuffle_host.h"
#include "../../include/curdle_g1.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#ifndef CG1_HD
#define CG1_HD inline
#endif
namespace cg1 {
#include "glv.h"
#include "fixed_digits.h"
#include "light_digits.h"
}

namespace cg1h {

typedef unsigned __int128 u128;

// ------------------------------------------------------------------ Jacobi symbol
// "posdivsteps": the safegcd recurrence with additions instead of subtractions, so f and g stay non-negative and the Jacobi symbol of
// (g / f) can be tracked through it (halving g flips the sign when f = 3, 5 mod 8; exchanging f and g flips it when both are 3 mod 4;
// adding a multiple of f to g changes nothing).  62 steps are run on the low 64 bits of f and g (exact there: after s halvings 64 - s
// low bits of g are still right, and the bookkeeping reads at most 3), collected in a 2 x 2 matrix with entries <= 2^62, which is then
// applied to the 7 x 62-bit limbs.  Every intermediate g is a weighted mean of the previous f and g, so both stay <= p.
// The number of batches has no proven bound for this variant: after MAX_BATCHES the caller decides by Euler's criterion instead
// (never seen in 10^7 random inputs: 381-bit operands finish in 13-17 batches).
namespace {

constexpr int JAC_LIMBS = 7;
constexpr uint64_t M62 = (1ull << 62) - 1;
constexpr int MAX_BATCHES = 40;

struct Trans { uint64_t u, v, q, r; };

inline int64_t posdivsteps_62(int64_t eta, uint64_t f0, uint64_t g0, Trans& t, unsigned& jacp) {
  uint64_t u = 1, v = 0, q = 0, r = 1;
  uint64_t f = f0, g = g0;
  unsigned jac = jacp;
  int i = 62;
  for (;;) {
    const int zeros = __builtin_ctzll(g | (~0ull << i));                // at most i: the sentinel stops the count
    g >>= zeros; u <<= zeros; v <<= zeros;
    eta -= zeros; i -= zeros;
    jac ^= (unsigned)(zeros & ((f >> 1) ^ (f >> 2)));                    // (2 / f) = -1  <=>  f = 3, 5 mod 8
    if (i == 0) break;
    uint64_t w, m;
    int limit;
    if (eta < 0) {
      eta = -eta;
      jac ^= (unsigned)((f & g) >> 1);                                    // reciprocity: both 3 mod 4
      uint64_t tmp;
      tmp = f; f = g; g = tmp;
      tmp = u; u = q; q = tmp;
      tmp = v; v = r; r = tmp;
      limit = ((int)eta + 1) > i ? i : ((int)eta + 1);
      m = (~0ull >> (64 - limit)) & 63u;
      w = (f * g * (f * f - 2)) & m;                                      // -g / f mod 64
    } else {
      limit = ((int)eta + 1) > i ? i : ((int)eta + 1);
      m = (~0ull >> (64 - limit)) & 15u;
      w = f + (((f + 1) & 4) << 1);                                       // 1 / f mod 16
      w = ((0 - w) * g) & m;                                              // -g / f mod 16
    }
    g += f * w; q += u * w; r += v * w;
  }
  t.u = u; t.v = v; t.q = q; t.r = r;
  jacp = jac;
  return eta;
}

inline void update_fg(uint64_t* f, uint64_t* g, const Trans& t, int len) {
  u128 cf = (u128)t.u * f[0] + (u128)t.v * g[0];
  u128 cg = (u128)t.q * f[0] + (u128)t.r * g[0];
  cf >>= 62; cg >>= 62;                                                    // the low 62 bits are zero by construction
  for (int i = 1; i < len; ++i) {
    cf += (u128)t.u * f[i] + (u128)t.v * g[i];
    cg += (u128)t.q * f[i] + (u128)t.r * g[i];
    f[i - 1] = (uint64_t)cf & M62; cf >>= 62;
    g[i - 1] = (uint64_t)cg & M62; cg >>= 62;
  }
  f[len - 1] = (uint64_t)cf;
  g[len - 1] = (uint64_t)cg;
}

// 6 x 64 -> 7 x 62
inline void to62(const uint64_t w[6], uint64_t o[JAC_LIMBS]) {
  for (int i = 0; i < JAC_LIMBS; ++i) {
    const unsigned bit = 62u * (unsigned)i, k = bit >> 6, sh = bit & 63u;
    uint64_t v = k < 6 ? w[k] >> sh : 0;
    if (sh > 2 && k + 1 < 6) v |= w[k + 1] << (64 - sh);
    o[i] = v & M62;
  }
}

// 2: did not finish
int jacobi_words(const uint64_t a[6]) {
  uint64_t f[JAC_LIMBS], g[JAC_LIMBS];
  for (int i = 0; i < JAC_LIMBS; ++i) f[i] = cg1::H_P62[i];
  to62(a, g);
  uint64_t nz = 0;
  for (int i = 0; i < JAC_LIMBS; ++i) nz |= g[i];
  if (!nz) return 0;
  int64_t eta = -1;
  unsigned jac = 0;
  int len = JAC_LIMBS;
  for (int count = 0; count < MAX_BATCHES; ++count) {
    Trans t;
    eta = posdivsteps_62(eta, f[0] | (f[1] << 62), g[0] | (g[1] << 62), t, jac);
    update_fg(f, g, t, len);
    if (f[0] == 1) {                                                       // f == 1: (g / 1) = 1 whatever g still is
      uint64_t rest = 0;
      for (int j = 1; j < len; ++j) rest |= f[j];
      if (!rest) return 1 - 2 * (int)(jac & 1u);
    }
    uint64_t gz = 0;
    for (int j = 0; j < len; ++j) gz |= g[j];
    if (!gz) return 0;                                                     // gcd = f != 1 (cannot happen for 0 < a < p, p prime)
    while (len > 2 && f[len - 1] == 0 && g[len - 1] == 0) --len;
  }
  return 2;
}

}  // namespace

int fe_jacobi(const fe& a) {
  const int j = jacobi_words(a.l);
  if (j != 2) return j;
  // Euler's criterion: a^((p-1)/2)
  if (fe_is_zero(a)) return 0;
  fe s;
  return fe_sqrt(a, s) ? 1 : -1;
}

static inline fe mkc(const uint64_t* w) { fe r; for (int i = 0; i < 6; ++i) r.l[i] = w[i]; return r; }

int g1_validate_compressed(const uint8_t in[48], bool* is_identity) {
  const uint8_t flags = in[0];
  if (is_identity) *is_identity = false;
  if (!(flags & 0x80)) return 1;
  if (flags & 0x40) { if (is_identity) *is_identity = true; return 0; }      // g1_decompress (host_g1.cpp): the identity whatever else is set
  uint8_t xb[48];
  memcpy(xb, in, 48);
  xb[0] &= 0x1F;
  fe x;
  if (!fe_from_be48(xb, x)) return 2;
  const fe rhs = fe_add(fe_mul(fe_sqr(x), x), mkc(cg1::H_B4));
  return fe_jacobi(rhs) < 0 ? 3 : 0;
}

// multiplication by |z| = 0xd201000000010000 (the BLS parameter's absolute value): 63 doublings + 5 additions
static jac mul_zabs(const jac& p) {
  constexpr uint64_t ZABS = 0xd201000000010000ull;
  jac q = p;
  for (int bit = 62; bit >= 0; --bit) {
    q = jac_dbl(q);
    if ((ZABS >> bit) & 1ull) q = jac_add(q, p);
  }
  return q;
}

bool g1_in_subgroup_fast(const fe& x, const fe& y) {
  const jac p = jac_from_affine(x, y);
  jac acc = mul_zabs(mul_zabs(p));                                          // [z^2] P
  const fe yneg = fe_neg(y);
  acc = jac_madd(acc, x, yneg);                                             // - P
  if (jac_is_identity(acc)) return false;                                   // [z^2] P == P and phi(P) == O is impossible for a finite P
  acc = jac_madd(acc, fe_mul(x, mkc(cg1::H_BETA)), yneg);                   // - phi(P)
  return jac_is_identity(acc);
}

// ------------------------------------------------------------------ one linear combination: interleaved width-5 NAF
namespace {

// width-5 NAF digits (odd, |d| <= 15) of a 256-bit little-endian integer; returns the number of digits
int wnaf5(const uint8_t k[32], int8_t naf[260]) {
  uint64_t w[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < 32; ++i) w[i >> 3] |= (uint64_t)k[i] << (8 * (i & 7));
  int len = 0;
  while (w[0] | w[1] | w[2] | w[3] | w[4]) {
    int d = 0;
    if (w[0] & 1) {
      d = (int)(w[0] & 31);
      if (d > 16) d -= 32;
      if (d > 0) {
        uint64_t b = (uint64_t)d;
        for (int i = 0; i < 5 && b; ++i) { const uint64_t t = w[i]; w[i] = t - b; b = t < b ? 1 : 0; }
      } else {
        uint64_t c = (uint64_t)(-d);
        for (int i = 0; i < 5 && c; ++i) { const uint64_t t = w[i] + c; c = t < c ? 1 : 0; w[i] = t; }
      }
    }
    naf[len++] = (int8_t)d;
    for (int i = 0; i < 4; ++i) w[i] = (w[i] >> 1) | (w[i + 1] << 63);
    w[4] >>= 1;
  }
  return len;
}

inline bool scalar_is(const uint8_t* s, uint8_t v) {
  if (s[0] != v) return false;
  for (int i = 1; i < 32; ++i) if (s[i]) return false;
  return true;
}

}  // namespace

jac lincomb_one(const aff* pts, const uint32_t* idx, const uint8_t* neg, const uint8_t* scalars32, size_t k) {
  jac units = jac_identity();                       // terms with coefficient 1: plain (mixed) additions
  struct Term { std::vector<int8_t> naf; jac tab[8]; };
  std::vector<Term> terms;
  terms.reserve(k);
  int maxlen = 0;
  for (size_t t = 0; t < k; ++t) {
    const aff& a = pts[idx[t]];
    if (a.inf) continue;
    const uint8_t* s = scalars32 + 32 * t;
    if (scalar_is(s, 0)) continue;
    const fe y = (neg && neg[t]) ? fe_neg(a.y) : a.y;
    if (scalar_is(s, 1)) { units = jac_madd(units, a.x, y); continue; }
    terms.emplace_back();
    Term& T = terms.back();
    int8_t naf[260];
    const int len = wnaf5(s, naf);
    T.naf.assign(naf, naf + len);
    maxlen = std::max(maxlen, len);
    T.tab[0] = jac_from_affine(a.x, y);
    const jac d2 = jac_dbl(T.tab[0]);
    for (int j = 1; j < 8; ++j) T.tab[j] = jac_add(T.tab[j - 1], d2);
  }
  jac acc = jac_identity();
  for (int i = maxlen - 1; i >= 0; --i) {
    acc = jac_dbl(acc);
    for (Term& T : terms) {
      if (i >= (int)T.naf.size()) continue;
      const int d = T.naf[i];
      if (d > 0) acc = jac_add(acc, T.tab[d >> 1]);
      else if (d < 0) acc = jac_add(acc, jac_neg(T.tab[(-d) >> 1]));
    }
  }
  return jac_add(acc, units);
}

static inline bool load_affine96(const uint8_t* rec, aff& o) {
  bool zero = true;
  for (int k = 0; k < 96 && zero; ++k) zero = rec[k] == 0;
  if (zero) { o.inf = true; o.x = fe_zero(); o.y = fe_zero(); return true; }
  o.inf = false;
  return fe_from_le48(rec, o.x) && fe_from_le48(rec + 48, o.y);
}

int lincomb_pool_jac(const uint8_t* bases_affine96, size_t n_bases, const uint32_t* offsets, const uint32_t* term_base, const uint8_t* term_scalars32,
                     const uint32_t* sel, size_t n_sel, jac* results, int n_threads) {
  if (n_sel == 0) return 0;
  // only the bases the selected combinations use are converted (a base costs one Montgomery product per coordinate)
  std::vector<aff> pts(n_bases);
  std::vector<uint8_t> loaded(n_bases, 0);
  size_t max_k = 0;
  for (size_t q = 0; q < n_sel; ++q) {
    const size_t j = sel ? sel[q] : q;
    max_k = std::max<size_t>(max_k, offsets[j + 1] - offsets[j]);
    for (size_t t = offsets[j]; t < offsets[j + 1]; ++t) {
      const uint32_t b = term_base[t] & 0x7fffffffu;
      if (b >= n_bases) return 1;
      if (!loaded[b]) { if (!load_affine96(bases_affine96 + 96 * (size_t)b, pts[b])) return 3; loaded[b] = 1; }
    }
  }
  // threads by the work at hand: a thread is worth waking for ~0.1 ms of arithmetic (~400 group operations), not for three additions
  if (n_threads <= 0) {
    double ops = 0;
    for (size_t q = 0; q < n_sel; ++q) {
      const size_t j = sel ? sel[q] : q;
      size_t heavy = 0, unit = 0;
      for (size_t t = offsets[j]; t < offsets[j + 1]; ++t) {
        const uint8_t* sc = term_scalars32 + 32 * t;
        bool small = sc[0] <= 1;
        for (int b = 1; b < 32 && small; ++b) small = sc[b] == 0;
        if (small) ++unit; else ++heavy;
      }
      ops += (heavy ? 255.0 : 0.0) + 52.0 * (double)heavy + (double)unit;
    }
    n_threads = (int)std::max<double>(1.0, std::min<double>(256.0, ops / 400.0));
  }
  // the one loop with per-thread scratch of the call's size (max_k): pool_for hands out the WORKERS, and they share a counter of their own
  const size_t workers = std::min<size_t>((size_t)n_threads, n_sel);
  std::atomic<size_t> next{0};
  cg1::pool_for(workers, (int)workers, [&](size_t) {
    std::vector<uint32_t> idx(max_k);
    std::vector<uint8_t> neg(max_k);
    for (size_t q; (q = next.fetch_add(1)) < n_sel;) {
      const size_t j = sel ? sel[q] : q;
      const size_t lo = offsets[j], k = offsets[j + 1] - lo;
      for (size_t t = 0; t < k; ++t) { idx[t] = term_base[lo + t] & 0x7fffffffu; neg[t] = (uint8_t)(term_base[lo + t] >> 31); }
      results[j] = lincomb_one(pts.data(), idx.data(), neg.data(), term_scalars32 + 32 * lo, k);
    }
  });
  return 0;
}

}  // namespace cg1h

// ------------------------------------------------------------------ C ABI (host-only entry points of the deferred evaluation)
namespace {

using cg1h::aff; using cg1h::fe; using cg1h::jac;
using cg1h::load_affine96;

}  // namespace

extern "C" void cg1_lincomb_write_outputs(const void* jac_results, size_t n_out, uint8_t* out_blobs144, uint8_t* out_affine96, uint8_t* out_comp48);

extern "C" {

int cg1_validate_compressed(const uint8_t* in48, int* is_identity) {
  if (!in48) return CG1_ERR_ARG;
  bool inf = false;
  const int rc = cg1h::g1_validate_compressed(in48, &inf);
  if (is_identity) *is_identity = inf ? 1 : 0;
  return rc == 0 ? CG1_OK : (rc == 3 ? CG1_ERR_NOT_ON_CURVE : CG1_ERR_ENCODING);
}

int cg1_fp_jacobi(const uint8_t* le48) {
  fe a;
  if (!le48 || !cg1h::fe_from_le48(le48, a)) return 2;
  return cg1h::fe_jacobi(a);
}

int cg1_batch_decompress_pool(const uint8_t* in48, size_t n, uint8_t* out_blobs144, uint8_t* out_affine96, int n_threads, size_t* bad_index) {
  if (n == 0) return CG1_OK;
  if (!in48) return CG1_ERR_ARG;
  std::atomic<size_t> bad{(size_t)-1};
  std::atomic<int> bad_rc{0};
  const size_t slice = 8, items = (n + slice - 1) / slice;
  if (n_threads <= 0) n_threads = (int)std::max<size_t>(1, std::min<size_t>(256, n / 8));        // ~0.1 ms of square roots per thread
  cg1::pool_for(items, n_threads, [&](size_t it) {
    for (size_t i = it * slice; i < std::min(n, it * slice + slice); ++i) {
      jac p;
      const int rc = cg1h::g1_decompress(in48 + 48 * i, false, p);
      if (rc != 0) {
        size_t cur = bad.load();
        while (i < cur && !bad.compare_exchange_weak(cur, i)) {}
        if (bad.load() == i) bad_rc.store(rc == 3 ? CG1_ERR_NOT_ON_CURVE : CG1_ERR_ENCODING);
        p = cg1h::jac_identity();
      }
      if (out_blobs144) memcpy(out_blobs144 + CG1_POINT_BYTES * i, &p, sizeof p);
      if (out_affine96) {
        uint8_t* o = out_affine96 + 96 * i;
        if (cg1h::jac_is_identity(p)) memset(o, 0, 96);
        else { cg1h::fe_to_le48(p.X, o); cg1h::fe_to_le48(p.Y, o + 48); }      // decoded points are in normal form (Z = 1)
      }
    }
  });
  if (bad.load() != (size_t)-1) { if (bad_index) *bad_index = bad.load(); return bad_rc.load() ? bad_rc.load() : CG1_ERR_ENCODING; }
  return CG1_OK;
}

int cg1_batch_subgroup_pool(const uint8_t* affine96, size_t n, uint8_t* out_flags, int n_threads) {
  if (n == 0) return CG1_OK;
  if (!affine96 || !out_flags) return CG1_ERR_ARG;
  std::atomic<int> bad{0};
  const size_t slice = 4, items = (n + slice - 1) / slice;
  if (n_threads <= 0) n_threads = (int)std::max<size_t>(1, std::min<size_t>(256, n / 3));        // ~0.1 ms of subgroup tests per thread
  cg1::pool_for(items, n_threads, [&](size_t it) {
    for (size_t i = it * slice; i < std::min(n, it * slice + slice); ++i) {
      aff a;
      if (!load_affine96(affine96 + 96 * i, a)) { bad.store(1); out_flags[i] = 0; continue; }
      out_flags[i] = a.inf ? 1 : (cg1h::g1_in_subgroup_fast(a.x, a.y) ? 1 : 0);
    }
  });
  return bad.load() ? CG1_ERR_ENCODING : CG1_OK;
}

// The pool path of cg1_lincomb_batch (msm_gpu.hip chooses between this and the GPU's batched MSM): see include/curdle_g1.h.
int cg1_lincomb_batch_pool(const uint8_t* bases_affine96, size_t n_bases, const uint32_t* offsets, size_t n_out, const uint32_t* term_base,
                           const uint8_t* term_scalars32, uint8_t* out_blobs144, uint8_t* out_affine96, uint8_t* out_comp48, int n_threads) {
  if (n_out == 0) return CG1_OK;
  if (!offsets || offsets[0] != 0) return CG1_ERR_ARG;
  const size_t T = offsets[n_out];
  if (T && (!bases_affine96 || !term_base || !term_scalars32)) return CG1_ERR_ARG;
  for (size_t j = 0; j < n_out; ++j) if (offsets[j] > offsets[j + 1]) return CG1_ERR_ARG;
  std::vector<jac> res(n_out);
  const int rc = cg1h::lincomb_pool_jac(bases_affine96, n_bases, offsets, term_base, term_scalars32, nullptr, n_out, res.data(), n_threads);
  if (rc) return rc == 3 ? CG1_ERR_ENCODING : CG1_ERR_ARG;
  cg1_lincomb_write_outputs(res.data(), n_out, out_blobs144, out_affine96, out_comp48);
  return CG1_OK;
}

// n results -> normalised blobs (Z = 1) / affine96 / compressed48 (each may be NULL) with ONE shared inversion
void cg1_lincomb_write_outputs(const void* jac_results, size_t n_out, uint8_t* out_blobs144, uint8_t* out_affine96, uint8_t* out_comp48) {
  const jac* res = static_cast<const jac*>(jac_results);
  std::vector<fe> xs(n_out), ys(n_out);
  std::vector<uint8_t> inf(n_out);
  cg1h::jac_batch_to_affine(res, n_out, xs.data(), ys.data(), inf.data());
  for (size_t j = 0; j < n_out; ++j) {
    if (out_blobs144) {
      const jac p = inf[j] ? cg1h::jac_identity() : cg1h::jac_from_affine(xs[j], ys[j]);
      memcpy(out_blobs144 + CG1_POINT_BYTES * j, &p, sizeof p);
    }
    if (out_affine96) {
      uint8_t* o = out_affine96 + 96 * j;
      if (inf[j]) memset(o, 0, 96);
      else { cg1h::fe_to_le48(xs[j], o); cg1h::fe_to_le48(ys[j], o + 48); }
    }
    if (out_comp48) cg1h::g1_compress_affine(xs[j], ys[j], inf[j] != 0, out_comp48 + 48 * j);
  }
}

// The endomorphism split the device digit kernels use (csrc/glv.h), one scalar: for the CPU tests.
void cg1_glv_split(const uint8_t* scalar32, uint8_t* k1_16, uint8_t* k2_16, int* neg1, int* neg2) {
  uint32_t k[8];
  memcpy(k, scalar32, 32);
  cg1::GlvParts o;
  cg1::glv_split(k, o);
  memcpy(k1_16, o.k1, 16);
  memcpy(k2_16, o.k2, 16);
  *neg1 = (int)o.neg1; *neg2 = (int)o.neg2;
}

// The signed 8-bit recoding of the fixed-base tables (csrc/fixed_digits.h: the function k_table_msm<FixedPlan> runs), one scalar: for the CPU tests.
void cg1_fixed_digits(const uint8_t* scalar32, int16_t* out32) {
  uint32_t k[8];
  memcpy(k, scalar32, 32);
  (void)cg1::fixed_digits(k, out32, 1);
}

// The signed narrow-window recoding of the light tables (csrc/light_digits.h: the function k_table_msm<LightPlan> runs), one scalar: for the CPU tests.
int cg1_light_digits(const uint8_t* scalar32, int16_t* out) {
  uint32_t k[8];
  memcpy(k, scalar32, 32);
  int8_t d[cg1::LT_WINDOWS];
  (void)cg1::light_digits(k, d, 1);
  for (int w = 0; w < cg1::LT_WINDOWS; ++w) out[w] = d[w];
  return cg1::LT_WINDOWS;
}

// The scalar schedule and the folds of the device prover of the inner-product argument (csrc/ipa_rounds.h: the functions k_ipa_step
// runs, one lane per term there, a loop here): for the CPU tests.
int cg1_ipa_round_emulate(int op, size_t n0, size_t len, uint8_t* c32, uint8_t* d32, uint8_t* kg32, uint8_t* kgp32, const uint8_t* kh32,
                          const uint8_t* challenge32, const uint8_t* r_c32, const uint8_t* r_d32, const uint32_t* g_index, const uint32_t* g_prime_index,
                          uint32_t h_index, uint32_t* out_term_base, uint8_t* out_term_scalars32, uint32_t* out_offsets) {
  using cg1fr::fr;
  auto pow2 = [](size_t v) { return v >= 2 && (v & (v - 1)) == 0; };
  if (op < 0 || op > 2 || !pow2(n0) || n0 > CG1_IPA_MAX_N || !pow2(len) || len > n0 || (op != 2 && len != n0) || !c32 || !d32 || !kg32 || !kgp32 || !kh32) return CG1_ERR_ARG;
  if (op != 2 && (!r_c32 || !r_d32)) return CG1_ERR_ARG;
  if (op == 1 && !challenge32) return CG1_ERR_ARG;
  if (op != 1 && (!g_index || !g_prime_index || !out_term_base || !out_term_scalars32 || !out_offsets)) return CG1_ERR_ARG;
  bool ok = true;
  auto load = [&](const uint8_t* src, size_t count) {
    std::vector<fr> v(count);
    for (size_t i = 0; i < count; ++i) ok = cg1fr::fr_from_le32(src + 32 * i, v[i]) && ok;
    return v;
  };
  std::vector<fr> c = load(c32, len), d = load(d32, len), kg = load(kg32, n0), kgp = load(kgp32, n0), kh = load(kh32, 1);
  std::vector<fr> ch = challenge32 ? load(challenge32, 1) : std::vector<fr>(), rc = op != 2 ? load(r_c32, n0) : std::vector<fr>(),
                  rd = op != 2 ? load(r_d32, n0) : std::vector<fr>();
  if (!ok) return CG1_ERR_ENCODING;
  cg1ipa::View v{c.data(), d.data(), kg.data(), kgp.data(), g_index, g_prime_index, h_index, (uint32_t)n0};
  const uint32_t h = (uint32_t)n0 / 2;
  if (op == 0) {
    std::vector<uint64_t> sc(4 * (size_t)cg1ipa::step1_terms((uint32_t)n0));
    for (uint32_t j = 0; j < n0; ++j) cg1ipa::step1_term(v, j, rc[j], rd[j], out_term_base, sc.data());
    memcpy(out_term_scalars32, sc.data(), sc.size() * 8);
    cg1ipa::step1_offsets((uint32_t)n0, 0, out_offsets);
    return CG1_OK;
  }
  if (op == 1) {
    for (uint32_t j = 0; j < n0; ++j) cg1ipa::blind_elem(v, j, ch[0], rc[j], rd[j]);
  } else {
    const uint32_t half = (uint32_t)len / 2;
    std::vector<uint64_t> sc(4 * (size_t)cg1ipa::round_terms((uint32_t)n0));
    fr sl = cg1fr::fr_zero(), sr = cg1fr::fr_zero();
    for (uint32_t t = 0; t < h; ++t) {
      fr pl, pr;
      cg1ipa::round_term(v, half, t, out_term_base, sc.data(), pl, pr);
      sl = cg1fr::fr_add(sl, pl); sr = cg1fr::fr_add(sr, pr);
    }
    cg1ipa::round_h_terms(v, kh[0], sl, sr, out_term_base, sc.data());
    memcpy(out_term_scalars32, sc.data(), sc.size() * 8);
    cg1ipa::round_offsets((uint32_t)n0, 0, out_offsets);
    if (challenge32) {
      if (cg1fr::fr_is_zero(ch[0])) return CG1_ERR_ARG;
      const fr ginv = cg1fr::fr_inv_binary(ch[0]);
      if (!cg1fr::fr_eq(ginv, cg1fr::fr_inv(ch[0]))) return CG1_ERR_ARG;          // the two inversions agree, or the test hears of it
      for (uint32_t t = 0; t < h; ++t) cg1ipa::fold_elem(v, half, t, ch[0], ginv);
      len = half;
    }
  }
  for (size_t i = 0; i < len; ++i) { cg1fr::fr_to_le32(c[i], c32 + 32 * i); cg1fr::fr_to_le32(d[i], d32 + 32 * i); }
  for (size_t i = 0; i < n0; ++i) { cg1fr::fr_to_le32(kg[i], kg32 + 32 * i); cg1fr::fr_to_le32(kgp[i], kgp32 + 32 * i); }
  return CG1_OK;
}

// The scalar schedule and the fold of the device prover of the same-MSM argument (csrc/same_msm_rounds.h: the functions k_smsm_step
// runs, one lane per term there, a loop here): for the CPU tests.  The two term arrays of a launch come back as ONE, in the
// transcript's order.
int cg1_same_msm_round_emulate(int op, size_t n0, size_t len, uint8_t* x32, uint8_t* k32, const uint8_t* challenge32, const uint8_t* r32,
                               const uint32_t* g_index, uint32_t* out_term_base, uint8_t* out_term_scalars32, uint32_t* out_offsets) {
  using cg1fr::fr;
  auto pow2 = [](size_t v) { return v >= 2 && (v & (v - 1)) == 0; };
  if (op < 0 || op > 2 || !pow2(n0) || n0 > CG1_SAME_MSM_MAX_N || !pow2(len) || len > n0 || (op != 2 && len != n0) || !x32 || !k32) return CG1_ERR_ARG;
  if (op != 2 && !r32) return CG1_ERR_ARG;
  if (op == 1 && !challenge32) return CG1_ERR_ARG;
  if (op != 1 && (!g_index || !out_term_base || !out_term_scalars32 || !out_offsets)) return CG1_ERR_ARG;
  bool ok = true;
  auto load = [&](const uint8_t* src, size_t count) {
    std::vector<fr> v(count);
    for (size_t i = 0; i < count; ++i) ok = cg1fr::fr_from_le32(src + 32 * i, v[i]) && ok;
    return v;
  };
  std::vector<fr> x = load(x32, len), k = load(k32, n0);
  std::vector<fr> ch = challenge32 ? load(challenge32, 1) : std::vector<fr>(), r = op != 2 ? load(r32, n0) : std::vector<fr>();
  if (!ok) return CG1_ERR_ENCODING;
  cg1smsm::View v{x.data(), k.data(), g_index, 0u, (uint32_t)n0};
  const uint32_t n = (uint32_t)n0, h = n / 2;
  std::vector<uint32_t> tba(n), tbl(2 * n);
  std::vector<uint64_t> sca(4 * (size_t)n), scl(8 * (size_t)n);
  // one array in the transcript's order: `lists` MSMs of `each` terms, list q from the A array (q % 3 == 0) or the T | U array
  auto merge = [&](uint32_t lists, uint32_t each) {
    for (uint32_t q = 0; q < lists; ++q) {
      const uint32_t g = q / 3, m = q % 3;
      const uint32_t* tb = m == 0 ? tba.data() + g * each : tbl.data() + (2 * g + m - 1) * each;
      const uint64_t* sc = m == 0 ? sca.data() + 4 * (size_t)g * each : scl.data() + 4 * (size_t)(2 * g + m - 1) * each;
      memcpy(out_term_base + (size_t)q * each, tb, 4 * (size_t)each);
      memcpy(out_term_scalars32 + 32 * (size_t)q * each, sc, 32 * (size_t)each);
      out_offsets[q] = q * each;
    }
    out_offsets[lists] = lists * each;
  };
  if (op == 0) {
    for (uint32_t j = 0; j < n; ++j) cg1smsm::begin_term(v, j, r[j], tba.data(), sca.data(), tbl.data(), scl.data());
    merge(3, n);
    return CG1_OK;
  }
  if (op == 1) {
    for (uint32_t j = 0; j < n; ++j) cg1smsm::blind_elem(v, j, ch[0], r[j]);
  } else {
    const uint32_t half = (uint32_t)len / 2;
    for (uint32_t t = 0; t < h; ++t) cg1smsm::round_term(v, half, t, tba.data(), sca.data(), tbl.data(), scl.data());
    merge(6, h);
    if (challenge32) {
      if (cg1fr::fr_is_zero(ch[0])) return CG1_ERR_ARG;
      const fr ginv = cg1fr::fr_inv_binary(ch[0]);
      if (!cg1fr::fr_eq(ginv, cg1fr::fr_inv(ch[0]))) return CG1_ERR_ARG;          // the two inversions agree, or the test hears of it
      for (uint32_t t = 0; t < h; ++t) cg1smsm::fold_elem(v, half, t, ch[0], ginv);
      len = half;
    }
  }
  for (size_t i = 0; i < len; ++i) cg1fr::fr_to_le32(x[i], x32 + 32 * i);
  for (size_t i = 0; i < n0; ++i) cg1fr::fr_to_le32(k[i], k32 + 32 * i);
  return CG1_OK;
}

// The formulas, the blinder completion and the term schedule of the device prover of the grand-product argument (csrc/gprod_rounds.h: the
// functions k_gprod_step runs -- a workgroup scan and an LDS tree there, loops here), with the two challenges given: for the CPU tests.
int cg1_gprod_emulate(size_t ell, size_t n_blinders, const uint8_t* gprod_result32, const uint8_t* vec_b32, const uint8_t* vec_c_blinders32,
                      const uint8_t* ipa_r32, const uint8_t* ipa_z_head32, const uint8_t* alpha32, const uint8_t* beta32, const uint32_t* g_index,
                      uint8_t* out_state32, uint8_t* out_scalars32, uint32_t* out_term_base, uint8_t* out_term_scalars32, uint32_t* out_offsets,
                      uint32_t* out_status) {
  using cg1fr::fr;
  const size_t nb = n_blinders, n0 = ell + nb;
  if (ell < 1 || nb < 2 || n0 < ell || (n0 & (n0 - 1)) != 0 || n0 > CG1_IPA_MAX_N) return CG1_ERR_ARG;
  if (!gprod_result32 || !vec_b32 || !vec_c_blinders32 || !ipa_r32 || !ipa_z_head32 || !alpha32 || !beta32 || !g_index || !out_state32 || !out_scalars32 ||
      !out_term_base || !out_term_scalars32 || !out_offsets || !out_status) return CG1_ERR_ARG;
  bool ok = true;
  auto load = [&](const uint8_t* src, size_t count) {
    std::vector<fr> v(count);
    for (size_t i = 0; i < count; ++i) ok = cg1fr::fr_from_le32(src + 32 * i, v[i]) && ok;
    return v;
  };
  const std::vector<fr> gres = load(gprod_result32, 1), b = load(vec_b32, n0), cbl = load(vec_c_blinders32, nb), r = load(ipa_r32, n0),
                        ch = load(alpha32, 1), bt = load(beta32, 1);
  std::vector<fr> z = load(ipa_z_head32, n0 - 2);
  if (!ok) return CG1_ERR_ENCODING;
  const uint32_t n = (uint32_t)n0, L = (uint32_t)ell;
  const fr alpha = ch[0], beta = bt[0];
  *out_status = 0;
  std::vector<fr> c(n), d(n), kg(n, cg1fr::fr_one()), kgp(n);
  std::vector<uint64_t> sc(4 * (size_t)5 * n);
  // ---- begin: the prefix products, the product, the terms of B' and C
  fr pre = cg1fr::fr_one();
  for (uint32_t i = 0; i < L; ++i) { c[i] = pre; pre = cg1fr::fr_mul(pre, b[i]); }
  for (uint32_t k = 0; k < nb; ++k) c[L + k] = cbl[k];
  if (!cg1fr::fr_eq(pre, gres[0])) *out_status |= cg1gprod::ST_BAD_PRODUCT;
  for (uint32_t j = 0; j < n; ++j) cg1gprod::begin_term(g_index, n, j, b[j], c[j], out_term_base, sc.data());
  // ---- step: r_p, the powers, vec_d, the coefficients, inner_prod
  fr r_p = cg1fr::fr_zero();
  for (uint32_t k = 0; k < nb; ++k) r_p = cg1fr::fr_add(r_p, cg1fr::fr_mul(cg1fr::fr_add(b[L + k], alpha), c[L + k]));
  fr beta_inv = cg1fr::fr_zero();
  if (cg1fr::fr_is_zero(beta)) *out_status |= cg1gprod::ST_ZERO_BETA;
  else {
    beta_inv = cg1fr::fr_inv_binary(beta);
    if (!cg1fr::fr_eq(beta_inv, cg1fr::fr_inv(beta))) return CG1_ERR_ARG;             // the two inversions agree, or the test hears of it
  }
  fr pw = cg1fr::fr_one(), pwi = beta_inv;
  for (uint32_t i = 0; i < L; ++i) {
    d[i] = cg1gprod::d_elem(b[i], beta, pw);
    kgp[i] = pwi;
    pw = cg1fr::fr_mul(pw, beta); pwi = cg1fr::fr_mul(pwi, beta_inv);
  }
  const fr beta_ell = pw, beta_ell1 = cg1fr::fr_mul(pw, beta);
  for (uint32_t k = 0; k < nb; ++k) { d[L + k] = cg1gprod::d_blinder(cg1fr::fr_add(b[L + k], alpha), beta_ell1); kgp[L + k] = pwi; }
  const fr ip = cg1gprod::inner_prod(r_p, gres[0], beta_ell, beta_ell1);
  // ---- the blinders' completion
  fr omega = cg1fr::fr_zero(), delta = cg1fr::fr_zero();
  for (uint32_t j = 0; j < n; ++j) {
    omega = cg1fr::fr_add(omega, cg1fr::fr_mul(r[j], d[j]));
    if (j + 2 < n) { omega = cg1fr::fr_add(omega, cg1fr::fr_mul(z[j], c[j])); delta = cg1fr::fr_add(delta, cg1fr::fr_mul(r[j], z[j])); }
  }
  const fr e = cg1gprod::blinder_denominator(r[n - 2], r[n - 1], c[n - 2], c[n - 1]);
  if (cg1fr::fr_is_zero(c[n - 2])) *out_status |= cg1gprod::ST_ZERO_C;
  if (cg1fr::fr_is_zero(e)) *out_status |= cg1gprod::ST_ZERO_DENOMINATOR;
  fr pen = cg1fr::fr_zero(), last = cg1fr::fr_zero();
  if (!(*out_status & (cg1gprod::ST_ZERO_C | cg1gprod::ST_ZERO_DENOMINATOR)))
    cg1gprod::blinder_finish(omega, delta, r[n - 2], c[n - 2], c[n - 1], e, cg1fr::fr_inv_binary(cg1fr::fr_mul(e, c[n - 2])), pen, last);
  z.push_back(pen); z.push_back(last);
  // ---- the terms of D, B_c, B_d
  cg1ipa::View v{c.data(), d.data(), kg.data(), kgp.data(), g_index, g_index, 0u, n};
  for (uint32_t j = 0; j < n; ++j)
    cg1gprod::step_term(v, j, j < L ? cg1fr::fr_sub(b[j], beta_inv) : cg1fr::fr_add(b[j], alpha), r[j], z[j], out_term_base + 2 * n, sc.data() + 4 * (size_t)2 * n);
  if (*out_status) return CG1_ERR_ARG;
  memcpy(out_term_scalars32, sc.data(), sc.size() * 8);
  for (uint32_t q = 0; q <= 5; ++q) out_offsets[q] = q * n;
  for (uint32_t j = 0; j < n; ++j) {
    cg1fr::fr_to_le32(c[j], out_state32 + 32 * (size_t)j); cg1fr::fr_to_le32(d[j], out_state32 + 32 * (size_t)(n + j));
    cg1fr::fr_to_le32(kgp[j], out_state32 + 32 * (size_t)(2 * n + j)); cg1fr::fr_to_le32(z[j], out_state32 + 32 * (size_t)(3 * n + j));
  }
  cg1fr::fr_to_le32(r_p, out_scalars32); cg1fr::fr_to_le32(ip, out_scalars32 + 32);
  return CG1_OK;
}

// The head of the device prover of the same-permutation argument: the host transcript head the entry runs (on a copy of the state: a
// refused call leaves it alone) and the formulas and term schedule of k_same_perm_begin (csrc/same_perm_rounds.h -- a workgroup scan
// there, a loop here): for the CPU tests.
int cg1_same_perm_emulate(size_t ell, size_t n_blinders, uint8_t* state208, const uint8_t* a48, const uint8_t* m48, const uint8_t* vec_a32, const uint32_t* perm,
                          const uint8_t* vec_a_blinders32, const uint8_t* vec_m_blinders32, const uint8_t* vec_c_blinders32, const uint32_t* g_index,
                          uint8_t* out_challenges32, uint8_t* out_b32, uint8_t* out_gprod_result32, uint32_t* out_term_base, uint8_t* out_term_scalars32,
                          uint32_t* out_offsets, uint32_t* out_status) {
  using cg1fr::fr;
  const size_t nb = n_blinders, n0 = ell + nb;
  if (ell < 1 || nb < 2 || n0 < ell || (n0 & (n0 - 1)) != 0 || n0 > CG1_IPA_MAX_N) return CG1_ERR_ARG;
  if (!state208 || !a48 || !m48 || !vec_a32 || !perm || !vec_a_blinders32 || !vec_m_blinders32 || !vec_c_blinders32 || !g_index || !out_challenges32 || !out_b32 ||
      !out_gprod_result32 || !out_term_base || !out_term_scalars32 || !out_offsets || !out_status) return CG1_ERR_ARG;
  for (size_t i = 0; i < ell; ++i)
    if (perm[i] >= ell) return CG1_ERR_ARG;
  bool ok = true;
  auto load = [&](const uint8_t* src, size_t count) {
    std::vector<fr> v(count);
    for (size_t i = 0; i < count; ++i) ok = cg1fr::fr_from_le32(src + 32 * i, v[i]) && ok;
    return v;
  };
  const std::vector<fr> va = load(vec_a32, ell), abl = load(vec_a_blinders32, nb), mbl = load(vec_m_blinders32, nb), cbl = load(vec_c_blinders32, nb);
  if (!ok) return CG1_ERR_ENCODING;
  uint8_t am[96];
  for (int q = 0; q < 2; ++q) {                             // as the transcript absorbs them: the identity re-serialised
    int inf = 0;
    const uint8_t* src = q == 0 ? a48 : m48;
    const int rc = cg1_validate_compressed(src, &inf);
    if (rc != CG1_OK) return rc;
    memcpy(am + 48 * q, src, 48);
    if (inf) { memset(am + 48 * q, 0, 48); am[48 * q] = 0xC0; }
  }
  // ---- same_perm_step1 [A, M], same_perm_step1 vec_a -> same_perm_alpha, same_perm_beta
  static const uint8_t step1[] = "same_perm_step1", l_alpha[] = "same_perm_alpha", l_beta[] = "same_perm_beta";
  cg1_merlin_append_list(state208, step1, 15, am, 48, 2);
  cg1_merlin_append_list(state208, step1, 15, vec_a32, 32, ell);
  cg1_merlin_challenge_scalar(state208, l_alpha, 15, out_challenges32);
  cg1_merlin_challenge_scalar(state208, l_beta, 14, out_challenges32 + 32);
  const std::vector<fr> ch = load(out_challenges32, 2);
  const uint32_t n = (uint32_t)n0, L = (uint32_t)ell;
  *out_status = 0;
  // ---- b | b_blinders, the prefix products, gprod_result, the terms of A', M', B', C
  std::vector<fr> b(n), c(n);
  for (uint32_t j = 0; j < L; ++j) b[j] = cg1sperm::factor(va[perm[j]], perm[j], ch[0], ch[1]);
  for (uint32_t k = 0; k < nb; ++k) b[L + k] = cg1sperm::blinder(abl[k], mbl[k], ch[0]);
  fr pre = cg1fr::fr_one();
  for (uint32_t i = 0; i < L; ++i) { c[i] = pre; pre = cg1fr::fr_mul(pre, b[i]); }
  for (uint32_t k = 0; k < nb; ++k) c[L + k] = cbl[k];
  std::vector<uint64_t> sc(4 * (size_t)cg1sperm::begin_terms(n));
  for (uint32_t j = 0; j < n; ++j)
    cg1sperm::begin_term(g_index, n, j, j < L ? va[perm[j]] : abl[j - L], j < L ? cg1fr::fr_from_u64(perm[j]) : mbl[j - L], b[j], c[j], out_term_base, sc.data());
  memcpy(out_term_scalars32, sc.data(), sc.size() * 8);
  cg1sperm::begin_offsets(n, 0, out_offsets);
  for (uint32_t j = 0; j < n; ++j) cg1fr::fr_to_le32(b[j], out_b32 + 32 * (size_t)j);
  cg1fr::fr_to_le32(pre, out_gprod_result32);
  return CG1_OK;
}

// The term schedule and the formulas of the device prover of the same-scalar block (csrc/same_scalar_rounds.h: the functions
// k_sscalar_step runs, one lane per element there, a loop here) and, given the ten encodings, its transcript step on the host: for the
// CPU tests.
int cg1_same_scalar_emulate(size_t ell, const uint8_t* vec_a32, const uint8_t* k32, const uint8_t* blinders32, const uint8_t* enc480, uint8_t* state208,
                            uint32_t* out_term_base, uint8_t* out_term_scalars32, uint32_t* out_offsets, uint8_t* out_alpha32, uint8_t* out_z96) {
  using cg1fr::fr;
  if (ell < 1 || ell > CG1_SAME_SCALAR_MAX_ELL) return CG1_ERR_ARG;
  if (!vec_a32 || !k32 || !blinders32 || !out_term_base || !out_term_scalars32 || !out_offsets || (enc480 && (!state208 || !out_alpha32 || !out_z96))) return CG1_ERR_ARG;
  bool ok = true;
  auto load = [&](const uint8_t* src, size_t count) {
    std::vector<fr> v(count);
    for (size_t i = 0; i < count; ++i) ok = cg1fr::fr_from_le32(src + 32 * i, v[i]) && ok;
    return v;
  };
  const std::vector<fr> va = load(vec_a32, ell), k = load(k32, 1), bl = load(blinders32, 5);          // bl: r_t r_u r_a r_b r_k
  if (!ok) return CG1_ERR_ENCODING;
  uint8_t enc[cg1sscalar::MSMS * 48];
  for (uint32_t q = 0; enc480 && q < cg1sscalar::MSMS; ++q) {          // as the transcript absorbs them: the identity re-serialised
    int inf = 0;
    const int rc = cg1_validate_compressed(enc480 + 48 * q, &inf);
    if (rc != CG1_OK) return rc;
    memcpy(enc + 48 * q, enc480 + 48 * q, 48);
    if (inf) { memset(enc + 48 * q, 0, 48); enc[48 * q] = 0xC0; }
  }
  const uint32_t L = (uint32_t)ell;
  std::vector<uint64_t> sc(4 * (size_t)cg1sscalar::terms(L));
  for (uint32_t j = 0; j < L; ++j) cg1sscalar::elem_terms(L, cg1sscalar::SHARED_BASES, j, va[j], k[0], bl[4], out_term_base, sc.data());
  for (uint32_t w = 0; w < 4; ++w) cg1sscalar::blinder_terms(L, w, bl[w], out_term_base, sc.data());
  memcpy(out_term_scalars32, sc.data(), sc.size() * 8);
  cg1sscalar::offsets(L, 0, out_offsets);
  if (!enc480) return CG1_OK;
  // ---- sameexp_points [R, S, T.T_1, T.T_2, U.T_1, U.T_2, A.T_1, A.T_2, B.T_1, B.T_2] -> same_scalar_alpha, then the responses
  static const uint8_t l_points[] = "sameexp_points", l_alpha[] = "same_scalar_alpha";
  cg1_merlin_append_list(state208, l_points, 14, enc, 48, cg1sscalar::MSMS);
  cg1_merlin_challenge_scalar(state208, l_alpha, 17, out_alpha32);
  const std::vector<fr> alpha = load(out_alpha32, 1);
  cg1fr::fr_to_le32(cg1sscalar::response(bl[4], k[0], alpha[0]), out_z96);
  cg1fr::fr_to_le32(cg1sscalar::response(bl[2], bl[0], alpha[0]), out_z96 + 32);
  cg1fr::fr_to_le32(cg1sscalar::response(bl[3], bl[1], alpha[0]), out_z96 + 64);
  return CG1_OK;
}

// The formulas and the term schedule of k_shuffle_begin, the first kernel of a whole shuffle proof proved on the device
// (csrc/shuffle_rounds.h: one lane per element there, a loop here; the same-scalar block's terms from csrc/same_scalar_rounds.h, one
// prover whose vec_R starts at light-table index 3): for the CPU tests.  Any ell in 1 .. CG1_SAME_SCALAR_MAX_ELL, so that a test can
// pass 256 elements, where a lane of the kernel owns two.
int cg1_shuffle_begin_emulate(size_t ell, const uint8_t* vec_a32, const uint32_t* perm, const uint8_t* k32, const uint8_t* blinders32, const uint8_t* vec_a_blinders32,
                              const uint32_t* gi_a, const uint32_t* gi_m, uint32_t* out_term_base, uint8_t* out_term_scalars32, uint32_t* out_offsets,
                              uint8_t* out_vec_x32, uint32_t* out_ss_term_base, uint8_t* out_ss_term_scalars32, uint32_t* out_ss_offsets) {
  using cg1fr::fr;
  if (ell < 1 || ell > CG1_SAME_SCALAR_MAX_ELL) return CG1_ERR_ARG;
  if (!vec_a32 || !perm || !k32 || !blinders32 || !vec_a_blinders32 || !gi_a || !gi_m || !out_term_base || !out_term_scalars32 || !out_offsets || !out_vec_x32 ||
      !out_ss_term_base || !out_ss_term_scalars32 || !out_ss_offsets) return CG1_ERR_ARG;
  for (size_t i = 0; i < ell; ++i)
    if (perm[i] >= ell) return CG1_ERR_ARG;
  bool ok = true;
  auto load = [&](const uint8_t* src, size_t count) {
    std::vector<fr> v(count);
    for (size_t i = 0; i < count; ++i) ok = cg1fr::fr_from_le32(src + 32 * i, v[i]) && ok;
    return v;
  };
  const std::vector<fr> va = load(vec_a32, ell), k = load(k32, 1), bl = load(blinders32, 5), abl = load(vec_a_blinders32, 2);      // bl: r_t r_u r_a r_b r_k
  if (!ok) return CG1_ERR_ENCODING;
  const uint32_t L = (uint32_t)ell, n = L + cg1shuffle::N_BLINDERS;
  std::vector<uint64_t> a64(4 * ell), abl64(8), sc(4 * (size_t)cg1shuffle::head_terms(n)), vx(4 * (size_t)n), ss_sc(4 * (size_t)cg1sscalar::terms(L));
  memcpy(a64.data(), vec_a32, 32 * ell); memcpy(abl64.data(), vec_a_blinders32, 64);
  for (uint32_t j = 0; j < n; ++j)
    cg1shuffle::head_term(gi_a, gi_m, n, L, j, cg1shuffle::x_elem(L, j, a64.data(), perm, abl64.data(), bl[0], bl[1]), out_term_base, sc.data(), vx.data());
  memcpy(out_term_scalars32, sc.data(), sc.size() * 8);
  memcpy(out_vec_x32, vx.data(), vx.size() * 8);
  cg1shuffle::head_offsets(n, 0, out_offsets);
  for (uint32_t j = 0; j < L; ++j) cg1sscalar::elem_terms(L, cg1sscalar::SHARED_BASES, j, va[j], k[0], bl[4], out_ss_term_base, ss_sc.data());
  for (uint32_t w = 0; w < 4; ++w) cg1sscalar::blinder_terms(L, w, bl[w], out_ss_term_base, ss_sc.data());
  memcpy(out_ss_term_scalars32, ss_sc.data(), ss_sc.size() * 8);
  cg1sscalar::offsets(L, 0, out_ss_offsets);
  return CG1_OK;
}

// The operations of fr.h as compiled for the HOST over items taken as given: the twin of cg1_probe_fr_ops (k_probe_fr, kernels_chain.h,
// has the layout), so that a test can hold the device's 32-bit-limb product and both inversions against these bytes.
int cg1_fr_ops_host(int op, const uint8_t* in, size_t n, uint8_t* out) {
  using cg1fr::fr;
  if (n == 0) return CG1_OK;
  if (op < 0 || op >= CG1_FR_OP_COUNT || !in || !out) return CG1_ERR_ARG;
  for (size_t i = 0; i < n; ++i) {
    const uint8_t* src = in + 64 * i;
    fr a, b, r = cg1fr::fr_zero();
    memcpy(a.l, src, 32); memcpy(b.l, src + 32, 32);
    uint64_t ok = 1;
    switch (op) {
      case CG1_FR_OP_MUL: r = cg1fr::fr_mul(a, b); break;
      case CG1_FR_OP_ADD: r = cg1fr::fr_add(a, b); break;
      case CG1_FR_OP_SUB: r = cg1fr::fr_sub(a, b); break;
      case CG1_FR_OP_NEG: r = cg1fr::fr_neg(a); break;
      case CG1_FR_OP_FROM_LE32: ok = cg1fr::fr_from_le32(src, r) ? 1 : 0; break;
      case CG1_FR_OP_FROM_LE64_WIDE: r = cg1fr::fr_from_le64_wide(src); break;
      case CG1_FR_OP_TO_LE32: cg1fr::fr_to_le32(a, reinterpret_cast<uint8_t*>(r.l)); break;
      case CG1_FR_OP_INV: r = cg1fr::fr_inv(a); break;
      case CG1_FR_OP_INV_BINARY: r = cg1fr::fr_inv_binary(a); break;
      default: r = cg1fr::fr_pow_u64(a, b.l[0]); break;                       // CG1_FR_OP_POW_U64
    }
    const uint64_t o[8] = {r.l[0], r.l[1], r.l[2], r.l[3], ok, 0, 0, 0};
    memcpy(out + 64 * i, o, 64);
  }
  return CG1_OK;
}

// The host twin of cg1_whisk_shuffle_front (capi_whisk_shuffle.h) for ONE prover, over the host G1 code (host_g1.cpp): the same
// refusals in the same order with the same texts (whisk_shuffle_host.h), the same layouts out.  For the CPU tests.
int cg1_whisk_shuffle_front_emulate(size_t ell, const uint8_t* trackers96, const uint32_t* perm, const uint8_t* k32, const uint8_t* vec_m_blinders32,
                                    const uint8_t* gh_affine96, uint8_t* out_rs_affine96, uint8_t* out_tu_affine96, uint8_t* out_post96, uint8_t* out_m_scalars32,
                                    uint8_t* out_m48, char* out_err256) {
  static const char* const who = "cg1_whisk_shuffle_front_emulate";
  char local[256];
  char* err = out_err256 ? out_err256 : local;
  err[0] = 0;
  if (!trackers96 || !perm || !k32 || !vec_m_blinders32 || !out_rs_affine96 || !out_tu_affine96 || !out_post96 || !out_m_scalars32 || (gh_affine96 && !out_m48)) {
    snprintf(err, 256, "%s: bad argument", who);
    return CG1_ERR_ARG;
  }
  if (const int rc = cg1whisk_host::check_shape(err, 256, who, ell)) return rc;
  if (const int rc = cg1whisk_host::check_inputs(err, 256, who, ell, 1, perm, k32, vec_m_blinders32)) return rc;
  const size_t n = ell + cg1whisk_host::N_BLINDERS;
  // ---- decode (unchecked: the decoder's leniency), then the subgroup test, each in tracker order
  std::vector<uint8_t> pts(2 * ell * CG1_POINT_BYTES), tmp(CG1_POINT_BYTES);          // vec_R | vec_S
  for (int pass = 0; pass < 2; ++pass)
    for (size_t i = 0; i < ell; ++i)
      for (int half = 0; half < 2; ++half) {
        uint8_t* dst = pass == 0 ? &pts[(half * ell + i) * CG1_POINT_BYTES] : tmp.data();
        const int rc = cg1_decompress(dst, trackers96 + 96 * i + 48 * half, pass);
        if (rc != CG1_OK) return cg1whisk_host::refuse_point(err, 256, who, 0, i, half, rc);
      }
  // ---- M = MSM(vec_G | vec_H, perm | vec_m_blinders), before anything is written
  std::vector<uint8_t> row(32 * n), m_enc(48);
  cg1whisk_host::m_scalar_row(ell, perm, vec_m_blinders32, row.data());
  if (gh_affine96) {
    uint8_t acc[CG1_POINT_BYTES], base[CG1_POINT_BYTES], term[CG1_POINT_BYTES];
    cg1_identity(acc);
    for (size_t j = 0; j < n; ++j) {
      const int rc = cg1_from_affine96(base, gh_affine96 + 96 * j, 1);
      if (rc != CG1_OK) { snprintf(err, 256, "%s: entry %zu of vec_G | vec_H is not a curve point (status %d)", who, j, rc); return rc; }
      cg1_mul(term, base, &row[32 * j]);
      cg1_add(acc, acc, term);
    }
    cg1_compress(m_enc.data(), acc);
  }
  // ---- the outputs
  cg1_batch_to_affine96(out_rs_affine96, pts.data(), 2 * ell);
  std::vector<uint8_t> tu(2 * ell * CG1_POINT_BYTES);
  for (size_t h = 0; h < 2; ++h)
    for (size_t i = 0; i < ell; ++i) {
      uint8_t* dst = &tu[(h * ell + i) * CG1_POINT_BYTES];
      cg1_mul(dst, &pts[(h * ell + perm[i]) * CG1_POINT_BYTES], k32);
      cg1_compress(out_post96 + 96 * i + 48 * h, dst);
    }
  cg1_batch_to_affine96(out_tu_affine96, tu.data(), 2 * ell);
  memcpy(out_m_scalars32, row.data(), 32 * n);
  if (gh_affine96) memcpy(out_m48, m_enc.data(), 48);
  return CG1_OK;
}

// The host twin of cg1_whisk_shuffle_draws_device (capi_whisk_shuffle.h): the same format (whisk_shuffle_host.h) over the host Keccak, the
// same refusals; no context, so a refusal carries no text.
int cg1_whisk_shuffle_draws(size_t ell, size_t n_provers, const uint8_t* seed32, uint64_t first_index, uint32_t* out_perm, uint8_t* out_scalars32) {
  if (!seed32 || !out_perm || !out_scalars32) return CG1_ERR_ARG;
  if (const int rc = cg1whisk_host::check_draws(nullptr, 0, "cg1_whisk_shuffle_draws", ell, n_provers, first_index)) return rc;
  const uint32_t L = (uint32_t)ell, P = (uint32_t)n_provers, D = cg1whisk_host::draw_count(L);
  for (uint32_t p = 0; p < P; ++p) {
    uint32_t* perm = out_perm + (size_t)p * L;
    for (uint32_t i = 0; i < L; ++i) perm[i] = i;
    for (uint32_t d = 0; d < D; ++d) {
      uint8_t msg[64], st[64];
      cg1whisk_host::draw_message(seed32, (uint32_t)(first_index + p), d, msg);
      cg1::shake256_block64(msg, 62, st);                      // (draw_message's byte 62 is the domain byte the helper sets)
      if (d + 1 < L) {
        uint64_t lo, hi;
        memcpy(&lo, st, 8); memcpy(&hi, st + 8, 8);
        const uint32_t i = L - 1 - d, j = cg1whisk_host::draw_mod_u128(lo, hi, i + 1);
        std::swap(perm[i], perm[j]);
      } else {
        cg1fr::fr_to_le32(cg1fr::fr_from_le64_wide(st), out_scalars32 + 32 * cg1whisk_host::draw_slot(L, P, p, d - (L - 1)));
      }
      cg1::wipe(msg, sizeof msg); cg1::wipe(st, sizeof st);
    }
  }
  return CG1_OK;
}

}  // extern "C"
