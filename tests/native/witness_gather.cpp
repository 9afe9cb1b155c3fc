// ASan/UBSan harness for the shuffle witness view (csrc/whisk_shuffle_host.h: ShuffleWitness::of_draws, ::gather) over a draw block whose
// every scalar names its own (prover, scalar number).  What a column must hold is written out here from the format's comment -- scalar
// number s runs through k (1), vec_m_blinders (4), vec_a_blinders (2), vec_c_blinders (4), ipa_r (n), ipa_z_head (n - 2), r_t r_u r_a r_b r_k
// (5), vec_r (n) -- and from draw_slot, which the device draws compile; nothing here asks the column table under test.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../curdleproofs_pie_amd/csrc/secret_wipe.h"
#include "../../curdleproofs_pie_amd/csrc/whisk_shuffle_host.h"

namespace W = cg1whisk_host;

static void encode(uint8_t* scalar32, uint32_t p, uint32_t s) {
  for (int b = 0; b < 32; ++b) scalar32[b] = (uint8_t)(0x40 + b);
  memcpy(scalar32, &p, 4); memcpy(scalar32 + 4, &s, 4);
}
static uint32_t perm_word(uint32_t p, uint32_t i) { return 0x5a000000u | (p << 12) | i; }

static int run(uint32_t ell, uint32_t P, const std::vector<size_t>& keep) {
  const uint32_t n = ell + 4, S = 3 * n + 14;
  if (W::draw_scalars(ell) != S) { printf("ell %u: draw_scalars is %u, not 3 n + 14\n", ell, W::draw_scalars(ell)); return 1; }
  // the block as the draws leave it: perm rows, then (on a 64-byte boundary) the scalars in the column layout
  const size_t at_scalars = ((size_t)P * ell * 4 + 63) / 64 * 64;
  std::vector<uint8_t> stage(at_scalars + (size_t)P * S * 32, 0xEE);
  for (uint32_t p = 0; p < P; ++p) {
    for (uint32_t i = 0; i < ell; ++i) { const uint32_t w = perm_word(p, i); memcpy(&stage[4 * ((size_t)p * ell + i)], &w, 4); }
    for (uint32_t s = 0; s < S; ++s) {
      const size_t slot = W::draw_slot(ell, P, p, s);
      if (slot >= (size_t)P * S) { printf("ell %u: draw_slot(%u, %u) = %zu lies outside the block\n", ell, p, s, slot); return 1; }
      encode(&stage[at_scalars + 32 * slot], p, s);
    }
  }
  // first scalar number and width of every column, in the order of the comment
  const uint32_t first[8] = {0, 1, 5, 7, 11, 11 + n, 9 + 2 * n, 14 + 2 * n}, width[8] = {1, 4, 2, 4, n, n - 2, 5, n};
  const W::ShuffleWitness all = W::ShuffleWitness::of_draws(stage.data(), ell, P);
  const size_t Q = keep.size();
  int bad = 0;
  {
    cg1::WipedBytes into;
    const W::ShuffleWitness g = all.gather(keep.data(), Q, into);
    if (Q == P && (g.perm != all.perm || g.col[0] != all.col[0] || !into.v.empty())) { printf("ell %u: the identity made a copy\n", ell); ++bad; }
    if (g.ell != ell || g.P != Q) { printf("ell %u: the gathered view says ell %zu, P %zu\n", ell, g.ell, g.P); ++bad; }
    for (size_t q = 0; q < Q; ++q) {
      const uint32_t p = (uint32_t)keep[q];
      for (uint32_t i = 0; i < ell; ++i)
        if (g.perm[q * ell + i] != perm_word(p, i)) { printf("ell %u Q %zu: perm row %zu entry %u is %08x\n", ell, Q, q, i, g.perm[q * ell + i]); ++bad; }
      for (int c = 0; c < 8; ++c)
        for (uint32_t j = 0; j < width[c]; ++j) {
          uint8_t want[32];
          encode(want, p, first[c] + j);
          if (memcmp(g.col[c] + 32 * (q * width[c] + j), want, 32) != 0) { printf("ell %u Q %zu: column %d row %zu scalar %u is not (%u, %u)\n", ell, Q, c, q, j, p, first[c] + j); ++bad; }
        }
    }
  }
  return bad;
}

int main() {
  const std::vector<std::vector<size_t>> keeps = {{0, 1, 2, 3, 4}, {}, {0}, {4}, {1, 3}, {0, 2, 4}};
  int bad = 0;
  for (uint32_t ell : {4u, 12u})
    for (const auto& keep : keeps) bad += run(ell, 5, keep);
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("sanitize ok\n");
  return 0;
}
