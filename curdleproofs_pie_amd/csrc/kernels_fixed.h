// k_table_msm: MSMs over a RESIDENT table of window multiples -- no doubling anywhere, the sum finished on the device.  One kernel body,
// instantiated per PLAN (what a table's records and digits are): FixedPlan here, for the tables of fixed bases described below, and
// LightPlan (kernels_light.h) for the light tables of bases that live for one proof.
// Part of the single translation unit csrc/msm_gpu.hip (included inside namespace cg1, after kernels_generator.h).
//
// The protocol's small MSMs run over points that never change (the CRS: crs.py:92-101), yet k_msm_small pays a full Pippenger pass --
// 37 windows, a bucket reduction per window, up to 255 doublings in the host Horner -- for the same points call after call.  Here the
// doublings are paid once per table: for bases B_0 .. B_{m-1}
//     tab[(b * GEN_WINDOWS + w) * GEN_HALF + (d - 1)] = d * 2^(8 w) * B_b        w = 0 .. 31,  d = 1 .. 128
// as prepared records (512 KiB per base; the layout and the builder of k_generator_mul's table of G, one base after the other), and a
// term k * B_b is the sum of at most 32 records picked by the signed digits of k (fixed_digits.h), negated where the digit or the
// term's sign bit says so.
//
// Grid = (slices of `slice` terms of one MSM, MSMs of the call); W = 8 or 16 waves per workgroup (the launch's choice, below):
//   digits   one lane per term: scalar < r and index < n_bases checked (a bad term sets the call's status word and contributes
//            nothing), the plan's digits (32 here) into LDS, window-major -- pair p = w * ns + t, so that the waves share the terms evenly whatever
//            windows the scalars leave empty (small scalars: only window 0)
//   sum      wave v adds the records of pairs v, v + W, ... one after the other; zero digits are skipped (wave-uniform)
//   tree     W waves -> 1 through LDS (log2 W levels)
//   join     several slices: partial sums to device memory; the LAST workgroup of the MSM to arrive (ticket, k_msm_small's pattern)
//            adds them, again W waves wide + the tree.  No workgroup waits for another; nothing spins.
//   export   the MSM's point as canonical XYZZ words into mapped host memory (the context's flag protocol: the last MSM to finish
//            publishes the status words and the sequence number), and / or as an XYZZ record for k_fixed_finish (affine96 /
//            compressed48 on the device, one inversion per output as at the end of k_generator_mul)
//
// Row form, not quads: every addition goes through ONE row_add (fp_row.h: the 14 limbs of a field element in 14 lanes, one addition
// per wave at a time).  The phase is a latency chain -- an IPA round is 4 x 65 terms = 8 320 additions, a dozen per wave once spread
// over the chip, plus the trees -- and what a dependent addition costs was measured with the very primitives (k_probe_add_chain,
// profiles/r05_rowlane_ab.txt): a wave of rows 1.7-1.8 us alone on its SIMD, 2.5 us with a second wave, against 5.4-5.5 / 9.9 us for
// a DPP quad and 12.3 us for one lane.  Quads add four points per instruction stream and so carry 3.5 times the additions per second
// once EVERY SIMD holds eight waves (3 516 against 924 per us), which takes ~60 000 additions in flight at once.  One round of one or
// of eight provers (8 320 / 66 560 additions) sits on the latency side, where rows win by 3x per step; only the largest shape measured,
// 64 provers in step (532 480 additions, ~0.6 ms at the chip's row rate), is where a quad variant would start to pay -- not built.
// The launch shape (slice, waves per workgroup) was then picked by timing this kernel itself (tools/gpu_fixed_base_timing.py --shapes ->
// profiles/r06_fixed_base_timing.txt: 4 x 65 terms 0.112 ms at 8 waves x 2 terms against 0.154 at 16 x 8 and 0.224 at 16 x 16; the
// rule is table_pick_shape, capi_fixed.h).  All additions are complete (row_add: identity,
// equal and opposite operands take the exact one-lane formulas).
#pragma once

static_assert(FIX_C == GEN_C && FIX_HALF == GEN_HALF && FIX_WINDOWS == GEN_WINDOWS, "the digit recoding and the table share one window plan");

constexpr uint32_t FX_WAVES = 16;                          // waves per workgroup, at most (a power of two; the launch may take fewer)
constexpr uint32_t FX_THREADS = FX_WAVES * 64;
constexpr uint32_t FX_MAX_SLICE = 128;                     // terms per workgroup, at most (the digits of a slice: 8 KiB of LDS)
constexpr uint32_t FX_MAX_TERMS = CG1_FIXED_MAX_TERMS;     // per MSM
constexpr uint32_t FX_MAX_MSMS = CG1_FIXED_MAX_MSMS;       // per call
constexpr uint32_t FX_BAD_SCALAR = 1u, FX_BAD_INDEX = 2u, FX_BAD_OFFSETS = 4u;      // bits of the call's status word

template <class Record>
struct TableArgs {
  const Record* tab;
  uint32_t n_bases;
  const uint32_t* term_base;              // per term: index into the table; bit 31 = the negated base
  const uint32_t* scalars;                // per term: 8 words, little-endian
  const uint32_t* offs;                   // M + 1 term offsets
  uint32_t M, n_terms, max_terms;         // max_terms: the longest MSM the grid was sized for
  uint32_t slice, Smax;                   // terms per workgroup; slices of the longest MSM (= gridDim.x)
  PointSum* partial;                      // [M][Smax]  (Smax > 1)
  uint32_t* counters;                     // [0, M): slice tickets; [M]: finished MSMs; [M + 1]: status bits.  Zero between calls.
  uint32_t* status_out;                   // 4 words: [0] = status bits of the call (device memory, or the record behind out_host's M points)
  PointWords* out_host;                   // nullable: M records in mapped host memory
  uint32_t* flag_host;
  uint32_t seq;
  PointSum* out_sum;                      // nullable: M XYZZ records (strictly normal limbs) for k_fixed_finish
};

// The fixed plan: 32 signed 8-bit digits per scalar (two bytes each in LDS: -128 .. 128), affine prepared records -- ZZ = ZZZ = one.
struct FixedPlan {
  using Record = PreparedPoint;
  using Digit = int16_t;
  static constexpr int WINDOWS = FIX_WINDOWS;
  static __device__ __forceinline__ void digits(const uint32_t s[8], Digit* dst, int stride) { (void)fixed_digits(s, dst, stride); }
  static __device__ __forceinline__ xyzz_row load(const Record* tab, uint32_t base, uint32_t window, uint32_t magnitude, const RowK& k) {
    const Record* rec = tab + ((size_t)base * GEN_WINDOWS + window) * GEN_HALF + (magnitude - 1u);
    xyzz_row o;
    o.X = row_load14(rec->x, k.lane16); o.Y = row_load14(rec->y, k.lane16); o.ZZ = k.one; o.ZZZ = k.one; o.inf = rec->flags & 1u;
    return o;
  }
};

// the one addition of the kernel, out of line: four call sites share ~5 KB of code (arguments and result travel in registers)
__device__ __attribute__((noinline)) xyzz_row fixed_add(xyzz_row a, xyzz_row b, RowK k) { return row_add(a, b, k); }

// W waves -> wave 0 (k_small_tree_row's LDS tree); every thread of the workgroup takes part
__device__ __forceinline__ xyzz_row fixed_tree(xyzz_row acc, PointSum* sh, uint32_t wv, uint32_t W, const RowK& k) {
  for (uint32_t d = W >> 1; d >= 1u; d >>= 1) {
    if (wv >= d && wv < 2u * d) row_store_sum(&sh[wv - d], acc, k.lane16);
    __syncthreads();
    if (wv < d) acc = fixed_add(acc, row_load_sum(&sh[wv], k.lane16), k);
    __syncthreads();
  }
  return acc;
}

// A plan is what differs between the tables: Record (the type of tab), Digit (the LDS element of a digit), WINDOWS, digits(s, dst, stride)
// and load(tab, base, window, magnitude, k) -> the record as a row.  Compile-time facts and inlined functions only: each instantiation
// is the kernel written out for its table.
template <class Plan>
__global__ void __launch_bounds__(FX_THREADS) k_table_msm(TableArgs<typename Plan::Record> a) {
  __shared__ typename Plan::Digit s_dig[FX_MAX_SLICE * Plan::WINDOWS];
  __shared__ uint32_t s_base[FX_MAX_SLICE];
  __shared__ PointSum s_sum[FX_WAVES / 2];
  __shared__ uint32_t s_ticket;

  const uint32_t tid = threadIdx.x, wv = tid >> 6, W = blockDim.x >> 6, sl = blockIdx.x, msm = blockIdx.y, M = a.M;
  uint32_t first = a.offs[msm], n = a.offs[msm + 1] - first;
  if (a.offs[msm + 1] < first || a.offs[msm + 1] > a.n_terms || n > a.max_terms) {       // never read past the term arrays
    if (tid == 0 && sl == 0) atomicOr(&a.counters[M + 1], FX_BAD_OFFSETS);
    first = 0; n = 0;
  }
  const uint32_t S = n ? (n + a.slice - 1u) / a.slice : 1u;                                 // an empty MSM: one workgroup exports the identity
  if (sl >= S) return;
  const uint32_t base = sl * a.slice;
  const uint32_t ns = n - base < a.slice ? n - base : a.slice;

  // ---- digits
  for (uint32_t t = tid; t < ns; t += blockDim.x) {
    const uint32_t i = first + base + t;
    uint32_t s[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = a.scalars[8ull * i + k];
    const uint32_t tb = a.term_base[i], idx = tb & 0x7fffffffu;
    uint32_t bad = 0;
    if (!fixed_scalar_below_r(s)) bad |= FX_BAD_SCALAR;
    if (idx >= a.n_bases) bad |= FX_BAD_INDEX;
    if (bad) {
      atomicOr(&a.counters[M + 1], bad);
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] = 0;
    }
    Plan::digits(s, &s_dig[t], (int)ns);
    s_base[t] = bad ? 0u : tb;
  }
  __syncthreads();

  // ---- sum: one record per non-zero digit
  const RowK k = row_constants();
  const uint32_t l = k.lane16;
  xyzz_row acc; acc.X = acc.Y = acc.ZZ = acc.ZZZ = 0; acc.inf = 1;
  const uint32_t npairs = ns * (uint32_t)Plan::WINDOWS;
#pragma unroll 1
  for (uint32_t p = wv; p < npairs; p += W) {
    const int d = __builtin_amdgcn_readfirstlane((int)s_dig[p]);
    if (d == 0) continue;
    const uint32_t w = p / ns, t = p - w * ns;
    const uint32_t tb = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_base[t]);
    xyzz_row o = Plan::load(a.tab, tb & 0x7fffffffu, w, (uint32_t)(d < 0 ? -d : d), k);
    if ((d < 0) != ((tb >> 31) != 0u)) o.Y = row_norm_pass(row_norm_pass(k.kp3 - o.Y, l), l);
    acc = fixed_add(acc, o, k);
  }
  acc = fixed_tree(acc, s_sum, wv, W, k);

  // ---- join the slices: the last workgroup of this MSM to arrive adds their partial sums
  if (S > 1u) {
    PointSum* mine = a.partial + (size_t)msm * a.Smax;
    if (wv == 0u) row_store_sum(mine + sl, acc, l);
    __threadfence();
    __syncthreads();
    if (tid == 0) s_ticket = atomicAdd(&a.counters[msm], 1u);
    __syncthreads();
    if (s_ticket != S - 1u) return;
    __threadfence();
    acc.X = acc.Y = acc.ZZ = acc.ZZZ = 0; acc.inf = 1;
#pragma unroll 1
    for (uint32_t s2 = wv; s2 < S; s2 += W) acc = fixed_add(acc, row_load_sum(mine + s2, l), k);
    acc = fixed_tree(acc, s_sum, wv, W, k);
  }
  if (wv != 0u) return;                                    // (past the last barrier)

  // ---- export
  if (a.out_sum) {
    const xyzz r = row_to_xyzz(acc, l);
    if (tid == 0) store_sum(a.out_sum + msm, r);
  }
  if (a.out_host) row_export4(acc, l, a.out_host + msm);
  __threadfence_system();                                  // the exporting lanes' stores are visible before the ticket is drawn
  if (tid == 0) {
    a.counters[msm] = 0;                                   // this MSM's ticket word is free for the next call
    if (atomicAdd(&a.counters[M], 1u) == M - 1u) {         // the last MSM of the call: status word, then the flag the host polls
      a.status_out[0] = atomicAdd(&a.counters[M + 1], 0u);
      a.status_out[1] = 0; a.status_out[2] = 0; a.status_out[3] = 0;
      a.counters[M] = 0; a.counters[M + 1] = 0;
      __threadfence_system();
      if (a.flag_host) __hip_atomic_store(a.flag_host, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// a^(p-2) with one limb per lane: fp_pow6's sliding window (width 3, ~380 squarings + ~96 multiplications) over row_mul, every row of
// the wave inverting its own element.  The same products in the same order as fp_inv, so the same value, limb for limb after fp_norm.
// An inversion is ONE dependent chain, and what it costs a lone wave is the instructions on that chain: ~150 per product here against
// ~470 for the one-lane fp_mul (fp_row.h) -- and between two rounds of a device-resident argument (kernels_ipa.h) the chain IS the
// kernel: measured in profiles/r07_ipa_device_timing.txt.
__device__ __noinline__ uint32_t row_inv(uint32_t a, const RowK k) {
  constexpr uint64_t e[6] = {H_INV_EXP[0], H_INV_EXP[1], H_INV_EXP[2], H_INV_EXP[3], H_INV_EXP[4], H_INV_EXP[5]};
  const uint32_t a2 = row_mul(a, a, k);
  const uint32_t t3 = row_mul(a, a2, k), t5 = row_mul(t3, a2, k), t7 = row_mul(t5, a2, k);
  auto bit = [&](int i) -> unsigned { return (unsigned)((e[i >> 6] >> (i & 63)) & 1u); };
  uint32_t r = k.one;
  bool started = false;
  int i = 383;
  while (i >= 0 && !bit(i)) --i;
#pragma unroll 1
  while (i >= 0) {
    if (!bit(i)) { r = row_mul(r, r, k); --i; continue; }
    int j = i >= 2 ? i - 2 : 0;
    while (!bit(j)) ++j;                                     // window [i .. j], odd value
    unsigned val = 0;
    for (int t = i; t >= j; --t) val = (val << 1) | bit(t);
    const uint32_t lo = (val & 2u) ? t3 : a, hi = (val & 2u) ? t7 : t5, m = (val & 4u) ? hi : lo;
    if (started) {
      for (int t = i; t >= j; --t) r = row_mul(r, r, k);
      r = row_mul(r, m, k);
    } else {
      r = m;
      started = true;
    }
    i = j - 1;
  }
  return r;
}

// The sums k_table_msm left on the device -> affine96 (standard words, zeros = identity) and / or compressed48: one ROW of a wave per
// output (four outputs per workgroup), one inversion each -- row_inv above -- and lane 0 of the row finishes on the one-lane form
// (k_generator_mul's tail).  A call whose status word is set writes nothing.
__global__ void __launch_bounds__(64) k_fixed_finish(const PointSum* __restrict__ sums, const uint32_t* __restrict__ status, uint32_t M,
                                                     uint32_t* __restrict__ out96, uint32_t* __restrict__ out48) {
  if (status[0] != 0u) return;                             // (uniform)
  const RowK rk = row_constants();
  const uint32_t i = blockIdx.x * 4u + rk.row;
  const xyzz acc = load_sum(sums + (i < M ? i : M - 1u));  // every lane of the wave takes part in the row products: no early exit
  const fp tinv = fp_norm(row_to_fp(row_inv(row_from_fp(fp_mul(acc.ZZ, acc.ZZZ), rk.lane16), rk)));
  if (i >= M || rk.lane16 != 0u) return;
  uint32_t o[24];
  for (int k = 0; k < 24; ++k) o[k] = 0;
  if (!acc.inf) {
    const fp t = tinv;
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
