// The lineage of a chain of Whisk shuffles PROVED over one tracker set (shuffle_chain.py: ShuffleChainProver, TrackerSet.evolve): where every
// pre and post tracker of every block comes from, worked out ahead of any point arithmetic.  Host only; one source for cg1_chain_lineage
// (csrc/shuffle_verify.cpp, the CPU tests drive it) and for the device entries (capi_chain_prove.h).
//
// Block j with permutation pi and secret k_j reads pre[t] = set[indices[t]] (all ell reads before its first write) and writes
// set[indices[t]] = k_j * pre[pi[t]], t = 0 .. ell - 1 in order.  Both halves of a tracker take the same scalar, so the current value of a
// slot is (origin slot, composite scalar): composite * (the tracker the ORIGIN slot held before the call).  A slot starts as (itself, 1).
// (k1 k2 mod r) * P == k2 * (k1 * P) holds for P of order r only, so a block is refused -- it writes nothing -- when an origin it reads is
// flagged: a point that did not decode (CG1_WHISK_SHUFFLE_NO_DECODE) before a point outside G1 (CG1_WHISK_SHUFFLE_NOT_G1), each in tracker
// order, as cg1_whisk_shuffle_prove_seeded reports them.  A derived value is never flagged: every block that wrote it read clean origins.
#pragma once
#include <cstdint>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#include "fr.h"
#include "secret_wipe.h"
#include "../../include/curdle_g1.h"

namespace cg1chain {

constexpr uint32_t NO_ORIGIN = 0xffffffffu;               // out_origin of a refused block's positions

// The refusals, before anything is written.  err (nullable) never holds a scalar.
inline int lineage_check(char* err, size_t err_len, const char* who, size_t n_slots, const uint32_t* indices, const uint32_t* perm, const uint8_t* k32, size_t n_blocks,
                         size_t ell) {
  auto say = [&](const char* what, size_t b) { if (err) snprintf(err, err_len, "%s: block %zu: %s", who, b, what); };
  if (ell == 0 || ell >= (1ull << 16) || n_slots == 0 || n_slots >= (1ull << 30) || n_blocks >= (1ull << 31) / (2 * ell)) {
    if (err) snprintf(err, err_len, "%s: ell in 1 .. 65535, a set of 1 .. 2^30 - 1 slots and fewer than 2^30 / ell blocks", who);
    return CG1_ERR_ARG; }
  std::vector<uint8_t> seen(ell);
  for (size_t b = 0; b < n_blocks; ++b) {
    memset(seen.data(), 0, ell);
    for (size_t t = 0; t < ell; ++t) {
      if (indices[b * ell + t] >= n_slots) { say("a slot index outside the set", b); return CG1_ERR_ARG; }
      const uint32_t m = perm[b * ell + t];
      if (m >= ell || seen[m]) { say("not a permutation of 0 .. ell - 1", b); return CG1_ERR_ARG; }
      seen[m] = 1;
    }
    uint64_t w[4];
    memcpy(w, k32 + 32 * b, 32);
    if (cg1fr::geq_r(w)) { say("k is >= r: scalar32 must be a canonical Fr element", b); return CG1_ERR_ENCODING; }
  }
  return CG1_OK;
}

// point_status: 2 n_slots bytes, r_G of slot s at 2 s and k_r_G at 2 s + 1: 0 = certified in G1, CG1_WHISK_SHUFFLE_NO_DECODE,
// CG1_WHISK_SHUFFLE_NOT_G1; only the slots a block reads at first touch are looked at.
// out_status / out_bad_at: n_blocks; out_origin: [n_blocks][2][ell], the origin slot of pre position t at [b][0][t] and of post position t at
// [b][1][t] (NO_ORIGIN for a refused block); out_scalar32: the composites in the same layout, canonical (zeros for a refused block);
// out_writers: (slot, b ell + t of its last write) for every slot written, slots ascending (room for min(n_slots, n_blocks ell) pairs).
// Each output may be null.  The arguments have passed lineage_check, but for point_status (another value: CG1_ERR_ARG, nothing written).
inline int lineage(size_t n_slots, const uint8_t* point_status, const uint32_t* indices, const uint32_t* perm, const uint8_t* k32, size_t n_blocks, size_t ell,
                   int32_t* out_status, uint32_t* out_bad_at, uint32_t* out_origin, uint8_t* out_scalar32, uint32_t* out_writers, size_t* out_n_writers) {
  using cg1fr::fr;
  for (size_t e = 0; e < n_blocks * ell; ++e)
    for (int half = 0; half < 2; ++half) {
      const uint8_t f = point_status[2 * (size_t)indices[e] + half];
      if (f != 0 && f != CG1_WHISK_SHUFFLE_NO_DECODE && f != CG1_WHISK_SHUFFLE_NOT_G1) return CG1_ERR_ARG;
    }
  struct Value { uint32_t origin; fr comp; };
  std::vector<Value> cur(n_slots), pre(ell);               // cur[s].origin == NO_ORIGIN: still (s, 1)
  for (size_t s = 0; s < n_slots; ++s) cur[s].origin = NO_ORIGIN;
  std::vector<int32_t> last(n_slots, -1);
  const fr one = cg1fr::fr_one();
  for (size_t b = 0; b < n_blocks; ++b) {
    const uint32_t* idx = indices + b * ell;
    const uint32_t* pm = perm + b * ell;
    constexpr uint32_t NONE = 0xffffffffu;
    uint32_t dec = NONE, g1 = NONE;
    for (size_t t = 0; t < ell; ++t) {                     // every read, before the block's first write
      const Value& v = cur[idx[t]];
      pre[t].origin = v.origin == NO_ORIGIN ? idx[t] : v.origin;
      pre[t].comp = v.origin == NO_ORIGIN ? one : v.comp;
      for (uint32_t half = 0; half < 2; ++half) {
        const uint8_t f = point_status[2 * (size_t)pre[t].origin + half];
        if (f == CG1_WHISK_SHUFFLE_NO_DECODE && dec == NONE) dec = (uint32_t)(2 * t) + half;
        if (f == CG1_WHISK_SHUFFLE_NOT_G1 && g1 == NONE) g1 = (uint32_t)(2 * t) + half;
      }
    }
    const int32_t st = dec != NONE ? CG1_WHISK_SHUFFLE_NO_DECODE : g1 != NONE ? CG1_WHISK_SHUFFLE_NOT_G1 : 0;
    if (out_status) out_status[b] = st;
    if (out_bad_at) out_bad_at[b] = st == 0 ? 0u : dec != NONE ? dec : g1;
    uint32_t* oo = out_origin ? out_origin + b * 2 * ell : nullptr;
    uint8_t* os = out_scalar32 ? out_scalar32 + b * 2 * ell * 32 : nullptr;
    if (st) {                                              // refused: nothing is written, later blocks read what was there
      if (oo) for (size_t t = 0; t < 2 * ell; ++t) oo[t] = NO_ORIGIN;
      if (os) memset(os, 0, 2 * ell * 32);
      continue;
    }
    fr k;
    cg1fr::fr_from_le32(k32 + 32 * b, k);                  // (below r: lineage_check)
    for (size_t t = 0; t < ell; ++t) {
      const Value& src = pre[pm[t]];
      Value post;
      post.origin = src.origin;
      post.comp = cg1fr::fr_mul(src.comp, k);
      if (oo) { oo[t] = pre[t].origin; oo[ell + t] = post.origin; }
      if (os) { cg1fr::fr_to_le32(pre[t].comp, os + 32 * t); cg1fr::fr_to_le32(post.comp, os + 32 * (ell + t)); }
      cur[idx[t]] = post;                                  // in order of t: the last write of a repeated index wins
      last[idx[t]] = (int32_t)(b * ell + t);
    }
    cg1::wipe(&k, sizeof k);
  }
  cg1::wipe(cur.data(), cur.size() * sizeof(Value)); cg1::wipe(pre.data(), pre.size() * sizeof(Value));
  if (out_n_writers) {
    size_t m = 0;
    for (size_t s = 0; s < n_slots; ++s)
      if (last[s] >= 0) {
        if (out_writers) { out_writers[2 * m] = (uint32_t)s; out_writers[2 * m + 1] = (uint32_t)last[s]; }
        ++m;
      }
    *out_n_writers = m;
  }
  return CG1_OK;
}

}  // namespace cg1chain
