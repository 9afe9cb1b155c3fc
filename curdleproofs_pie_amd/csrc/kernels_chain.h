// The skeleton of a step kernel of an argument proved as ONE launch chain (kernels_ipa.h, kernels_same_msm.h, kernels_gprod.h, kernels_same_scalar.h): one workgroup per prover,
// between two k_table_msm / k_fixed_finish launches.  Shared by every argument: the transcript on lane 0 -- cg1merlin::Machine over the
// prover's OWN 208-byte state in device memory, absorbing the encodings k_fixed_finish left and drawing the step's challenge (that lane
// is the serial part of a step: Keccak permutations, a rejection-sampled draw, the inversion) -- the status of the launch before, the
// final scalars, lane 0's shader clocks.  An argument adds its phases, op tables, proof slots and *_rounds.h.
// Part of the single translation unit csrc/msm_gpu.hip (after kernels_merlin.h).
#pragma once
#include "chain_rounds.h"

namespace cg1chain {
using cg1merlin::COp;
using cg1merlin::LANES;
using cg1merlin::Machine;

constexpr uint32_t INV_NONE = 0, INV_BINARY = 1, INV_FERMAT = 2;      // which inverse of its challenge a step wants

struct StepLds {                             // a step kernel's transcript block
  uint32_t sponge[52 * LANES];
  uint32_t drawn[8 * LANES];
  uint32_t labels[5 * 8];
  uint32_t inf[12];
  alignas(16) COp ops[8];                    // (Machine::advance loads a record as one uint4)
  fr ch[2];                                  // the step's challenge | its inverse
};

__device__ __noinline__ fr inv_fermat(const fr& a) { return cg1fr::fr_inv(a); }
__device__ __noinline__ fr inv_binary(const fr& a) { return cg1fr::fr_inv_binary(a); }

// The Fr probe (cg1_probe_fr_ops, capi_rows_probes.h): one lane per item runs ONE operation of fr.h as compiled for the device -- the
// 32-bit-limb product, the two inversions through the very wrappers the steps call -- over a 64-byte item, 64 bytes out: the result in
// bytes 0..31, fr_from_le32's boolean as a word at byte 32.  mul, add, sub, neg, inv, inv_binary take and return raw Montgomery words
// (mul: any 256-bit first operand); pow_u64: the exponent at byte 32.  The host twin is cg1_fr_ops_host (lazy_host.cpp).
enum : int { FROP_MUL = CG1_FR_OP_MUL, FROP_ADD = CG1_FR_OP_ADD, FROP_SUB = CG1_FR_OP_SUB, FROP_NEG = CG1_FR_OP_NEG, FROP_FROM_LE32 = CG1_FR_OP_FROM_LE32,
             FROP_FROM_LE64_WIDE = CG1_FR_OP_FROM_LE64_WIDE, FROP_TO_LE32 = CG1_FR_OP_TO_LE32, FROP_INV = CG1_FR_OP_INV, FROP_INV_BINARY = CG1_FR_OP_INV_BINARY,
             FROP_POW_U64 = CG1_FR_OP_POW_U64, FROP_COUNT = CG1_FR_OP_COUNT };      // include/curdle_g1.h
__global__ void __launch_bounds__(64) k_probe_fr(const uint8_t* __restrict__ in, uint32_t n, int op, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint8_t* src = in + 64 * (size_t)i;                       // (items are 64-byte aligned: the entry point allocates the buffers)
  const uint64_t* w = reinterpret_cast<const uint64_t*>(src);
  const fr a{{w[0], w[1], w[2], w[3]}}, b{{w[4], w[5], w[6], w[7]}};
  fr r = cg1fr::fr_zero();
  uint32_t ok = 1;
  if (op == FROP_MUL) r = cg1fr::fr_mul(a, b);
  else if (op == FROP_ADD) r = cg1fr::fr_add(a, b);
  else if (op == FROP_SUB) r = cg1fr::fr_sub(a, b);
  else if (op == FROP_NEG) r = cg1fr::fr_neg(a);
  else if (op == FROP_FROM_LE32) ok = cg1fr::fr_from_le32(src, r) ? 1u : 0u;
  else if (op == FROP_FROM_LE64_WIDE) r = cg1fr::fr_from_le64_wide(src);
  else if (op == FROP_TO_LE32) cg1fr::fr_to_le32(a, reinterpret_cast<uint8_t*>(r.l));
  else if (op == FROP_INV) r = inv_fermat(a);
  else if (op == FROP_INV_BINARY) r = inv_binary(a);
  else r = cg1fr::fr_pow_u64(a, b.l[0]);
  uint64_t* o = reinterpret_cast<uint64_t*>(out + 64 * (size_t)i);
  o[0] = r.l[0]; o[1] = r.l[1]; o[2] = r.l[2]; o[3] = r.l[3]; o[4] = ok; o[5] = 0; o[6] = 0; o[7] = 0;
}

__device__ inline void label(uint32_t* dst, const char* s, uint32_t n) {          // label words, little-endian, zero-padded to 32 bytes
  for (uint32_t j = 0; j < 8u; ++j) dst[j] = 0u;
  for (uint32_t j = 0; j < n; ++j) dst[j >> 2] |= (uint32_t)(uint8_t)s[j] << ((j & 3u) * 8u);
}
__device__ inline COp op(uint32_t kind, uint32_t label, uint32_t llen, uint32_t len, uint32_t data_off, uint32_t out_off) {
  return COp{kind | (label << 8) | (llen << 16), len, data_off, out_off};
}

// The transcript of one step, called by the whole workgroup once lane 64 has written s.labels and s.ops[0 .. nops): the program runs
// over data row `row`, its draws go to `orow` (32 bytes each) and the first of them, the step's challenge, to s.ch[0]; s.ch[1] is its
// inverse where `inv` asks for one; *second (optional) receives a second drawn scalar.  status_b (optional): a second launch before.
// ck (optional): the prover's four clock words -- transcript | inversions | whole steps that emit terms (step_clock) | steps counted.
__device__ __forceinline__ void transcript_step(StepLds& s, uint8_t* st, uint32_t nops, const uint8_t* row, uint8_t* orow, const uint32_t* status_a,
                                       const uint32_t* status_b, uint32_t* chain_status, uint32_t inv, fr* second, uint32_t* ck) {
  const uint32_t tid = threadIdx.x;
  if (tid < 50u) s.sponge[tid * LANES] = reinterpret_cast<const uint32_t*>(st)[tid];
  if (tid == 64u) {
    s.inf[0] = 0xC0u;                                                   // the canonical encoding of the identity: C0 00 .. 00
    for (int j = 1; j < 12; ++j) s.inf[j] = 0u;
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0u) {
    const uint32_t bad = status_a[0] | (status_b ? status_b[0] : 0u);
    if (bad != 0u) atomicOr(chain_status, bad);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    Machine m;
    m.w = s.sponge; m.drawn = s.drawn; m.labels = s.labels; m.consts = reinterpret_cast<const uint8_t*>(s.inf);
    m.reset(st);
    bool done = false;
    for (;;) {
      bool blocked = false;
      if (!m.advance(s.ops, nops, row, orow, done, blocked)) break;
      cg1merlin::keccak_words(m.w);
      m.pos = 0; m.pos_begin = 0;
    }
    st[200] = (uint8_t)m.pos; st[201] = (uint8_t)m.pos_begin; st[202] = (uint8_t)m.cur_flags;
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    const fr ch = load_le(reinterpret_cast<const uint64_t*>(orow));
    s.ch[0] = ch;
    if (second) *second = load_le(reinterpret_cast<const uint64_t*>(orow + 32));
    if (inv != INV_NONE) s.ch[1] = inv == INV_FERMAT ? inv_fermat(ch) : inv_binary(ch);
    const unsigned long long t2 = __builtin_amdgcn_s_memtime();
    if (ck) {
      ck[0] += (uint32_t)(t1 - t0);
      if (inv != INV_NONE) ck[1] += (uint32_t)(t2 - t1);
      ck[3] += 1u;
    }
  }
  __threadfence_block();
  __syncthreads();
  if (tid < 50u) reinterpret_cast<uint32_t*>(st)[tid] = s.sponge[tid * LANES];
}

__device__ inline void put_scalar(uint32_t* dst, const fr& v) {       // a final scalar into the proof: 32 canonical bytes at a word address
  uint64_t w[4];
  cg1fr::fr_to_le32(v, reinterpret_cast<uint8_t*>(w));
  for (int k = 0; k < 4; ++k) { dst[2 * k] = (uint32_t)w[k]; dst[2 * k + 1] = (uint32_t)(w[k] >> 32); }
}
__device__ inline void step_clock(uint32_t* ck, unsigned long long t_in) {        // lane 0, at the end of a step that emitted terms
  if (ck) ck[2] += (uint32_t)(__builtin_amdgcn_s_memtime() - t_in);
}

}  // namespace cg1chain
