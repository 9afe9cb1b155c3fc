// The one way host code clears a secret: cg1::wipe (a memset the optimiser may not drop), cg1::WipedBytes (host staging that is wiped on
// every exit path) and the one-block SHAKE256 draw the seeded entries share, whose sponge state is wiped before it returns.  Included by
// the .hip unit and by the host-only sources alike.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/curdle_g1.h"

namespace cg1 {
inline void wipe(void* p, size_t n) {
  memset(p, 0, n);
  __asm__ __volatile__("" : : "r"(p) : "memory");          // the stores above are observable: none of them is dead
}
struct WipedBytes {
  std::vector<uint8_t> v;
  ~WipedBytes() { if (!v.empty()) wipe(v.data(), v.size()); }
};
// out64 = the first 64 bytes of SHAKE256(msg), len <= 135: one rate block, one permutation (cg1_keccak_f1600, merlin.cpp)
inline void shake256_block64(const uint8_t* msg, size_t len, uint8_t out64[64]) {
  alignas(8) uint8_t st[200] = {0};
  memcpy(st, msg, len);
  st[len] ^= 0x1F;
  st[135] ^= 0x80;
  cg1_keccak_f1600(st);
  memcpy(out64, st, 64);
  wipe(st, sizeof st);
}
}  // namespace cg1
