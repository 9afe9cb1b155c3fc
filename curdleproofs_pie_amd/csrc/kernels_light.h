// Light tables: window multiples of VARIABLE bases, built on the device in two launches, and k_light_msm over them -- no doubling at MSM time.
// Part of the single translation unit csrc/msm_gpu.hip (included inside namespace cg1, after kernels_fixed.h).
//
// A cg1_fixed table (kernels_fixed.h) costs 512 KiB and ~0.35 ms per base: right for the CRS, which lives as long as the process, and
// unaffordable for bases that live for ONE proof -- vec_T and vec_U of the same-MSM argument (curdleproofs.py:124-136: R k and S k), 2 n
// points that each enter lg n + 1 MSMs once the round challenges fold into the scalars.  A light table pays a base's doublings once per
// proof with narrow windows: c = LT_C bits (light_digits.h), for bases B_0 .. B_{m-1}
//     tab[(b * LT_WINDOWS + w) * LT_HALF + (d - 1)] = d * 2^(c w) * B_b        w = 0 .. LT_WINDOWS - 1,  d = 1 .. 2^(c-1)
// as full XYZZ records (PointSum: 256 B; c = 4: 64 x 8 records = 128 KiB per base).  XYZZ and not affine, so that the build needs no
// inversion; the limbs are what row_store_sum leaves (nearly normal), and only row code reads them back.  Every record carries its own
// infinity flag: an all-zero base is the identity and so are all its entries, and a base of small order has identities among its
// multiples (the order-3 point (0, 2): 3 B = O).
//
// Build (exact for EVERY point of the curve: row_dbl is complete -- the curve has no point of order 2 -- and row_add takes the exact
// one-lane formulas for equal and opposite operands):
//   k_light_chain       one wave per base walks B, 2^c B, 2^(2c) B, ...: c (LT_WINDOWS - 1) dependent doublings, 252 at c = 4 -- the
//                       latency of the build (1.25 us each measured for this kernel: 315 us / 252, profiles/r08_light_table_kernels.txt)
//   k_light_multiples   one wave per (base, window): Q = 2^(c w) B is there; 2 Q = dbl(Q), 3 Q = 2 Q + Q, 4 Q = dbl(2 Q), ... one
//                       operation per record, the earlier multiples kept by the wave in row form (five words per lane and point).  The
//                       row arithmetic itself spills: the record shows 716 B of scratch here and 780 B in k_light_msm
// One wave per RECORD, each walking its own double-and-add from Q (depth 3 to 4 at c = 4), would shorten the second chain from 7 steps
// to 4 at 22 operations per window instead of 7 -- and already one proof's table (256 bases x 64 windows = 16 384 waves, sixteen per
// SIMD) fills the chip, where the number of operations is what is paid: not built.
//
// k_light_msm is k_fixed_msm over these records: the same grid (slices, MSMs), digits in LDS window-major, one row_add per non-zero
// digit, the LDS tree, the ticketed slice join, the same exports and the same status bits -- it shares fixed_add, fixed_tree and
// k_fixed_finish.  No workgroup waits for another; nothing spins.
#pragma once

struct LightArgs {
  const PointSum* tab;
  uint32_t n_bases;
  const uint32_t* term_base;              // per term: index into the table; bit 31 = the negated base
  const uint32_t* scalars;                // per term: 8 words, little-endian
  const uint32_t* offs;                   // M + 1 term offsets
  uint32_t M, n_terms, max_terms;         // max_terms: the longest MSM the grid was sized for
  uint32_t slice, Smax;                   // terms per workgroup; slices of the longest MSM (= gridDim.x)
  PointSum* partial;                      // [M][Smax]  (Smax > 1)
  uint32_t* counters;                     // [0, M): slice tickets; [M]: finished MSMs; [M + 1]: status bits.  Zero between calls.
  uint32_t* status_out;                   // 4 words: [0] = status bits of the call
  PointWords* out_host;                   // nullable: M records in mapped host memory
  uint32_t* flag_host;
  uint32_t seq;
  PointSum* out_sum;                      // nullable: M XYZZ records (strictly normal limbs) for k_fixed_finish
};

__device__ __forceinline__ size_t light_record(uint32_t b, uint32_t w, uint32_t mag) {      // index of |d| = mag, window w, base b
  return ((size_t)b * LT_WINDOWS + w) * LT_HALF + (mag - 1u);
}

// bases: n affine96 records (standard form; all-zero = the identity), already checked to be curve points.  Grid = n, one wave each.
__global__ void __launch_bounds__(64) k_light_chain(const uint32_t* __restrict__ bases96, uint32_t n, PointSum* __restrict__ tab) {
  const uint32_t b = blockIdx.x;
  if (b >= n) return;
  const RowK k = row_constants();
  const uint32_t l = k.lane16;
  uint32_t r2 = 0;
#pragma unroll
  for (int t = 0; t < NL; ++t) r2 = l == (uint32_t)t ? fp_r2().l[t] : r2;
  uint32_t wd[24], any = 0;
  for (int t = 0; t < 24; ++t) { wd[t] = bases96[24ull * b + t]; any |= wd[t]; }
  xyzz_row q;
  q.X = row_mul(row_from_fp(fp_from_words(wd), l), r2, k);
  q.Y = row_mul(row_from_fp(fp_from_words(wd + 12), l), r2, k);
  q.ZZ = k.one; q.ZZZ = k.one; q.inf = any ? 0u : 1u;
  if (q.inf) q.X = q.Y = q.ZZ = q.ZZZ = 0;
#pragma unroll 1
  for (uint32_t w = 0; w < (uint32_t)LT_WINDOWS; ++w) {
    if (w) {
#pragma unroll 1
      for (int i = 0; i < LT_C; ++i) q = row_dbl(q, k);
    }
    row_store_sum(tab + light_record(b, w, 1u), q, l);
  }
}

// Grid = n * LT_WINDOWS, one wave per (base, window): records d = 2 .. LT_HALF from record 1.
__global__ void __launch_bounds__(64) k_light_multiples(PointSum* __restrict__ tab, uint32_t n) {
  const uint32_t b = blockIdx.x / (uint32_t)LT_WINDOWS, w = blockIdx.x - b * (uint32_t)LT_WINDOWS;
  if (b >= n) return;
  const RowK k = row_constants();
  const uint32_t l = k.lane16;
  PointSum* rec = tab + light_record(b, w, 1u);
  xyzz_row T[LT_HALF];                                     // T[d - 1] = d Q
  T[0] = row_load_sum(rec, l);
#pragma unroll
  for (int d = 2; d <= LT_HALF; ++d) {
    T[d - 1] = (d & 1) ? fixed_add(T[d - 2], T[0], k) : row_dbl(T[d / 2 - 1], k);      // (d - 1) Q = +-Q only for a base of small order: exact
    row_store_sum(rec + (d - 1), T[d - 1], l);
  }
}

__global__ void __launch_bounds__(FX_THREADS) k_light_msm(LightArgs a) {
  __shared__ int8_t s_dig[FX_MAX_SLICE * LT_WINDOWS];
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
    (void)light_digits(s, &s_dig[t], (int)ns);
    s_base[t] = bad ? 0u : tb;
  }
  __syncthreads();

  // ---- sum: one record per non-zero digit
  const RowK k = row_constants();
  const uint32_t l = k.lane16;
  xyzz_row acc; acc.X = acc.Y = acc.ZZ = acc.ZZZ = 0; acc.inf = 1;
  const uint32_t npairs = ns * (uint32_t)LT_WINDOWS;
#pragma unroll 1
  for (uint32_t p = wv; p < npairs; p += W) {
    const int d = __builtin_amdgcn_readfirstlane((int)s_dig[p]);
    if (d == 0) continue;
    const uint32_t w = p / ns, t = p - w * ns;
    const uint32_t tb = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_base[t]);
    xyzz_row o = row_load_sum(a.tab + light_record(tb & 0x7fffffffu, w, (uint32_t)(d < 0 ? -d : d)), l);
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
