// What the *_rounds.h of every argument proved as a device launch chain share (ipa_rounds.h, same_msm_rounds.h): canonical scalars in,
// the terms of the next table-MSM launch out.  One source for the device and the host, like the headers that include it.
#pragma once
#include "fr.h"

namespace cg1chain {
using cg1fr::fr;

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

}  // namespace cg1chain
