// The Fr half of the inner-product argument's prover (ipa.py:97-151) with the bases held FIXED: the scalar schedule of every MSM launch
// and the folds between two launches.  One source for the device (kernels_ipa.h: one lane per term) and the host (lazy_host.cpp:
// cg1_ipa_round_emulate, for the CPU tests) -- the way fixed_digits.h is shared.
//
// The reference folds the bases every round (G = G_L + gamma G_R).  Here a prover keeps, per ORIGINAL index j, the product kG[j] /
// kGp[j] of the challenges of the rounds in which j sat in the right half (prover_kernels.ipa_rounds_many has the derivation), and a
// round's MSM over a folded half becomes an MSM over n0 / 2 table bases with the coefficients multiplied into the scalars.  With the
// current length 2 * half, lane t = b * half + i (b: which block of 2 * half original indices, i < half) owns
//     jl = b * 2 half + i  (current position i, the left half)        jr = jl + half  (current position half + i, the right half)
// and emits one term of each of the round's four MSMs, in the order the transcript absorbs their results:
//     L_C  base G[jr]   scalar c[i]        kG[jr]        (+ the term  H  <c_L, d_R> kH  at the end)
//     L_D  base G'[jl]  scalar d[half + i] kGp[jl]
//     R_C  base G[jl]   scalar c[half + i] kG[jl]        (+ the term  H  <c_R, d_L> kH)
//     R_D  base G'[jr]  scalar d[i]        kGp[jr]
// kGp starts at the caller's G' coefficients (grand_prod.py:64-71 as scalars) or 1; kH is beta: crs_H * beta is never a point.
// A prover's terms are contiguous: [L_C: h + 1][L_D: h][R_C: h + 1][R_D: h] with h = n0 / 2, every round.
#pragma once
#include "fr.h"

namespace cg1ipa {
using cg1fr::fr;

struct View {                                // one prover's state (Montgomery form) and its table indices
  fr* c; fr* d;                              // the current vectors: positions [0, len)
  fr* kG; fr* kGp;                           // per original index, n0 each
  const uint32_t* gi; const uint32_t* gpi;   // table indices of crs_G_vec / crs_G_prime_vec, n0 each
  uint32_t hi;                               // table index of crs_H
  uint32_t n0;
};

CG1FR_HD uint32_t round_terms(uint32_t n0) { return 2u * n0 + 2u; }
CG1FR_HD uint32_t step1_terms(uint32_t n0) { return 2u * n0; }
// term offsets of a prover whose first term is `first`: 5 values for a round, 3 for step 1 (B_c over G, B_d over G')
CG1FR_HD void round_offsets(uint32_t n0, uint32_t first, uint32_t* o) {
  const uint32_t h = n0 / 2u;
  o[0] = first; o[1] = o[0] + h + 1u; o[2] = o[1] + h; o[3] = o[2] + h + 1u; o[4] = o[3] + h;
}
CG1FR_HD void step1_offsets(uint32_t n0, uint32_t first, uint32_t* o) { o[0] = first; o[1] = first + n0; o[2] = first + 2u * n0; }

// term `slot` of the prover's term arrays (tb: table index, bit 31 = negated base -- never set here; sc: 4 words per canonical scalar)
CG1FR_HD void put_term(uint32_t* tb, uint64_t* sc, uint32_t slot, uint32_t base, const fr& k) {
  uint64_t w[4];
  cg1fr::fr_to_le32(k, reinterpret_cast<uint8_t*>(w));
  tb[slot] = base;
  for (int i = 0; i < 4; ++i) sc[4u * slot + i] = w[i];
}
CG1FR_HD fr load_le(const uint64_t* src) {    // a canonical scalar (validated by the caller) -> Montgomery form
  uint64_t w[4] = {src[0], src[1], src[2], src[3]};
  fr v;
  (void)cg1fr::fr_from_le32(reinterpret_cast<const uint8_t*>(w), v);
  return v;
}

// step 1, lane j < n0:  B_c = MSM(G, r_c),  B_d = MSM(G', r_d)  (ipa.py:97-98)
CG1FR_HD void step1_term(const View& v, uint32_t j, const fr& rc, const fr& rd, uint32_t* tb, uint64_t* sc) {
  put_term(tb, sc, j, v.gi[j], rc);
  put_term(tb, sc, v.n0 + j, v.gpi[j], cg1fr::fr_mul(rd, v.kGp[j]));
}
// ipa.py:107-109, lane j < n0
CG1FR_HD void blind_elem(const View& v, uint32_t j, const fr& alpha, const fr& rc, const fr& rd) {
  v.c[j] = cg1fr::fr_add(rc, cg1fr::fr_mul(alpha, v.c[j]));
  v.d[j] = cg1fr::fr_add(rd, cg1fr::fr_mul(alpha, v.d[j]));
}
// a round's terms, lane t < n0 / 2 (ipa.py:126-129).  pl / pr: this lane's share of <c_L, d_R> / <c_R, d_L> (zero outside block 0)
CG1FR_HD void round_term(const View& v, uint32_t half, uint32_t t, uint32_t* tb, uint64_t* sc, fr& pl, fr& pr) {
  const uint32_t h = v.n0 / 2u, b = t / half, i = t - b * half, jl = b * 2u * half + i, jr = jl + half;
  const fr cl = v.c[i], cr = v.c[half + i], dl = v.d[i], dr = v.d[half + i];
  put_term(tb, sc, t, v.gi[jr], cg1fr::fr_mul(cl, v.kG[jr]));
  put_term(tb, sc, h + 1u + t, v.gpi[jl], cg1fr::fr_mul(dr, v.kGp[jl]));
  put_term(tb, sc, 2u * h + 1u + t, v.gi[jl], cg1fr::fr_mul(cr, v.kG[jl]));
  put_term(tb, sc, 3u * h + 2u + t, v.gpi[jr], cg1fr::fr_mul(dl, v.kGp[jr]));
  if (b == 0u) { pl = cg1fr::fr_mul(cl, dr); pr = cg1fr::fr_mul(cr, dl); }
  else { pl = cg1fr::fr_zero(); pr = cg1fr::fr_zero(); }
}
// the two H terms, once the inner products are summed
CG1FR_HD void round_h_terms(const View& v, const fr& kH, const fr& ip_l, const fr& ip_r, uint32_t* tb, uint64_t* sc) {
  const uint32_t h = v.n0 / 2u;
  put_term(tb, sc, h, v.hi, cg1fr::fr_mul(ip_l, kH));
  put_term(tb, sc, 3u * h + 1u, v.hi, cg1fr::fr_mul(ip_r, kH));
}
// ipa.py:142-146 with the bases left alone, lane t < n0 / 2: positions [0, half) of c and d are the folded vectors afterwards.
// In place: lane t reads positions i and half + i and writes position i only.
CG1FR_HD void fold_elem(const View& v, uint32_t half, uint32_t t, const fr& gamma, const fr& gamma_inv) {
  const uint32_t b = t / half, i = t - b * half, jr = b * 2u * half + half + i;
  v.kG[jr] = cg1fr::fr_mul(v.kG[jr], gamma);
  v.kGp[jr] = cg1fr::fr_mul(v.kGp[jr], gamma_inv);
  if (b == 0u) {
    v.c[i] = cg1fr::fr_add(v.c[i], cg1fr::fr_mul(gamma_inv, v.c[half + i]));
    v.d[i] = cg1fr::fr_add(v.d[i], cg1fr::fr_mul(gamma, v.d[half + i]));
  }
}

// 1 / a by Kaliski's almost-inverse (0 -> 0): a binary extended Euclid whose loop only shifts, adds and subtracts -- no reduction mod r
// inside -- and leaves a^-1 2^k (r bits <= k <= 2 r bits); the power of two goes away with two Montgomery products at the end.
// The round's challenge is public, so the data-dependent loop leaks nothing, and as ONE dependent chain on one lane its ~400 steps of
// word arithmetic take 0.12 ms against 0.50 for the 380 Montgomery products of a^(r-2) (cg1fr::fr_inv): DESIGN.md section 10 has
// both, timed.  Input and output in Montgomery form: with A = a R the loop gives A^-1 2^k = a^-1 R^-1 2^k, and
// a^-1 R = that * 2^(512 - k) = mont(that, mont(2^(512 - k), R^2)).
CG1FR_HD fr fr_inv_binary(const fr& a) {
  if (cg1fr::fr_is_zero(a)) return a;
  uint64_t u[4] = {cg1::H_FR[0], cg1::H_FR[1], cg1::H_FR[2], cg1::H_FR[3]};
  uint64_t w[4] = {a.l[0], a.l[1], a.l[2], a.l[3]};
  uint64_t x[4] = {0, 0, 0, 0}, y[4] = {1, 0, 0, 0};       // x, y < 2 r < 2^256 throughout
  uint32_t k = 0;
  while ((w[0] | w[1] | w[2] | w[3]) != 0) {
    const bool u_even = !(u[0] & 1), w_even = !(w[0] & 1);
    bool gt = false;                                        // u > w
    for (int i = 3; i >= 0; --i) if (u[i] != w[i]) { gt = u[i] > w[i]; break; }
    // which of the four steps: halve u | halve w | u <- (u - w) / 2 | w <- (w - u) / 2; the other side's cofactor doubles.
    // Two explicit calls, not a pointer chosen at run time: the four numbers stay in registers on the device.
    const bool on_u = u_even || (!w_even && gt), odd = !u_even && !w_even;
    auto step = [odd](uint64_t (&big)[4], const uint64_t (&small)[4], uint64_t (&acc)[4], uint64_t (&dbl)[4]) {
      if (odd) {
        cg1fr::u128 bw = 0, cy = 0;
        for (int i = 0; i < 4; ++i) {
          const cg1fr::u128 dlt = (cg1fr::u128)big[i] - small[i] - bw; big[i] = (uint64_t)dlt; bw = (dlt >> 64) & 1;
          cy += (cg1fr::u128)acc[i] + dbl[i]; acc[i] = (uint64_t)cy; cy >>= 64;
        }
      }
      for (int i = 0; i < 3; ++i) big[i] = (big[i] >> 1) | (big[i + 1] << 63);
      big[3] >>= 1;
      for (int i = 3; i > 0; --i) dbl[i] = (dbl[i] << 1) | (dbl[i - 1] >> 63);
      dbl[0] <<= 1;
    };
    if (on_u) step(u, w, x, y);
    else step(w, u, y, x);
    ++k;
  }
  if (cg1fr::geq_r(x)) cg1fr::sub_r(x);
  fr inv{{x[0], x[1], x[2], x[3]}};
  inv = cg1fr::fr_neg(inv);                                 // r - x = A^-1 2^k mod r, 255 <= k <= 510
  uint32_t e = 512u - k;                                    // 2 .. 257
  fr two_e{{0, 0, 0, 0}};
  const uint32_t eb = e > 254u ? 254u : e;                  // 2^e as a plain integer below r, the rest by doublings
  two_e.l[eb >> 6] = (uint64_t)1 << (eb & 63u);
  const fr r2{{cg1::H_FR_R2[0], cg1::H_FR_R2[1], cg1::H_FR_R2[2], cg1::H_FR_R2[3]}};
  fr out = cg1fr::fr_mul(inv, cg1fr::fr_mul(two_e, r2));
  for (; e > eb; --e) out = cg1fr::fr_add(out, out);
  return out;
}

}  // namespace cg1ipa
