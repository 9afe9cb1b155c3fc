// Host side of the MSM engine, part 2: the call planner.  Pure functions of the switches and a call's sizes -- no HIP call, no context:
// who serves a call (route_*), every number its launch chain derives (plan_regime_a / plan_regime_b) and the word that says which
// reduction-tail kernels it launches (tail_word).  host_chains.h launches what these say; cg1_msm_call_describe answers without a GPU.
// Part of the single translation unit csrc/msm_gpu.hip (included there, in this order; not a stand-alone header).
#pragma once

namespace cg1 {

// c > 0: uniform windows of width c (nwin = 255 / c + 1).  c < 0: a BALANCED plan with cmax = -c: the 256 bit positions
// are cut into nwin = ceil(256 / cmax) windows of width cmax (the low ones) or cmax - 1, so the top window keeps
// >= cmax - 2 scalar bits and the recoding carry never leaves it (scalars are < 2^255).
// glv: the same over the 128 bit positions of the halves of the endomorphism split (glv.h: magnitudes < 0.68 * 2^127).
static WinPlan make_plan(int c, bool glv = false) {
  WinPlan pl;
  const int bits = glv ? 127 : 255;
  pl.glv = glv ? 1 : 0;
  if (c > 0) { pl.cmax = c; pl.nwin = bits / c + 1; pl.n_hi = pl.nwin; }
  else {
    const int cm = -c, nw = (bits + 1 + cm - 1) / cm;
    pl.cmax = cm; pl.nwin = nw; pl.n_hi = bits + 1 - nw * (cm - 1);
    if (pl.n_hi < 0) pl.n_hi = 0;        // nw windows of width cm - 1 already cover every position (128 positions at cm = 14: 10 x 13): all narrow
  }
  return pl;
}

int pick_window(size_t n) {
  // Only widths whose TOP window still holds >= min(c-1, 7) scalar bits (255 = (nwin-1)*c + t): with t = 2..3 all
  // n terms of that window fall into <= 8 buckets.  Thresholds from tools/gpu_window_sweep.py on MI355X.
  if (n <= 128) return 4;        // t = 3
  if (n <= 8192) return 8;       // t = 7
  return 16;                     // t = 15
}

// window_c = 0: the plan per input size (tools/gpu_window_sweep.py on MI355X).  The 2-D bucket reduction costs two EC additions
// per BUCKET, the accumulation one per (term, window): mid-size inputs want fewer, fuller buckets than c = 16 gives them.
static int pick_plan_c(size_t n, int auto_plan) {
  const int c = pick_window(n);
  if (!auto_plan || c != 16) return c;
  if (n <= (1u << 14)) return -12;
  if (n <= (3u << 15)) return -13;
  if (n <= (3u << 16)) return -15;
  return 16;
}

// The window width k_msm_small runs a call of n terms with (uniform signed windows; 2^(c-1) <= 256 buckets fit one workgroup's
// LDS sort; 5 is left out: its top window would hold nothing but the recoding carry).  Chosen so that a slice of <= 256 terms puts
// a handful of entries into a bucket: every EC addition of the kernel is a ~10 us step of a dependent chain, and the reduction costs
// ~log2(buckets) + 4 of them per window whatever n is, so few buckets (64 at c = 7) beat the wider windows the entry count alone
// would suggest (measured, profiles/r04_small_msm.txt: n = 627 at c = 9 waits 232 us for the GPU, at c = 7 ...).
// (windows x slices must stay within ONE round of workgroups for a single MSM -- SM_ONE_ROUND = the chip's 256 CUs, a workgroup of
// k_msm_small fills one: 1 391 terms at c = 7 are 222 workgroups and take 0.35 ms, 2 048 are 296 = two rounds and take 0.47, more than
// the launch chain's 0.40 (profiles/r04_small_msm.txt) -- so from 1 537 terms on the plan is c = 8: 32 windows x 8 slices = 256)
static int pick_small_c(size_t n) {
  if (n <= 24) return 4;
  if (n <= 96) return 6;
  if (n <= 6 * SM_SLICE) return 7;
  return 8;
}

int pick_window_batched(size_t n_avg, bool glv) {
  const int bits = glv ? 127 : 255;
  if (glv) n_avg *= 2;                                 // entries per MSM: both halves of every term
  int best = 4; double best_cost = 1e300;
  for (int c = 4; c <= 9; ++c) {                       // NB <= 256: a group's counting sort fits one block's LDS
    if (bits % c == 0) continue;                       // top window would hold only the recoding carry: one hot bucket
    int nwin = bits / c + 1;
    double NB = (double)(1u << (c - 1));
    double cost = (double)nwin * ((double)n_avg + 1.4 * (2.0 * NB + 3.0 * NB / 8.0)) + 1.4 * (double)bits;
    if (cost < best_cost) { best_cost = cost; best = c; }
  }
  return best;
}
int pick_window_batched(size_t n_avg) { return pick_window_batched(n_avg, false); }

// ------------------------------------------------------------------ who serves a call
// (the values of cg1_msm_call_describe's out_engine: include/curdle_g1.h CG1_ENGINE_*)
enum Engine { ENGINE_NONE = 0, ENGINE_SMALL = 1, ENGINE_CHAIN_A = 2, ENGINE_TWO_CHAINS_A = 3, ENGINE_CHAIN_B = 4, ENGINE_TWO_CHAINS_B = 5 };
enum SrcKind { SRC_AFFINE96 = 0, SRC_BLOBS = 1, SRC_PREPARED = 2 };      // PtSrc::Kind's values (host_chains.h)

struct Route {
  int rc = CG1_OK; char err[96] = {0};  // a refusal, with the context's message
  Engine engine = ENGINE_NONE;          // NONE: nothing to launch (no terms)
  int c = 0;                            // the plan's width as cg1_get_timings reports it (negative: a balanced plan)
  bool glv = false;                     // the endomorphism split is on
  WinPlan plan;                         // (k_msm_small: make_plan(c, glv), uniform)
  Route& refuse(const char* fmt, int a = 0, int b = 0) { rc = CG1_ERR_ARG; snprintf(err, sizeof err, fmt, a, b); return *this; }
};

// does k_msm_small take `nn` entries (n terms, or the 2n of the split) in one round of workgroups at width c (0: its own choice)?
static bool small_fits_one(size_t nn, int c, bool sglv) {
  if (nn > SM_MAX_N || !(c == 0 || (c >= 4 && c <= 9 && c != 5))) return false;
  return (size_t)((sglv ? 127 : 255) / (c ? c : pick_small_c(nn)) + 1) * ((nn + SM_SLICE - 1) / SM_SLICE) <= SM_ONE_ROUND;
}

// One MSM of n terms (cg1_msm_device and its kin).  c = 0: automatic plan; 4..16: uniform windows; -16..-4: the balanced plan with cmax = -c.
static Route route_msm_call(const MsmSwitches& sw, size_t n, int c, int rank, int world, int src_kind) {
  Route r;
  if (n == 0) return r;
  if (n >= (1ull << 31)) return r.refuse("n too large");
  if (world < 1 || world > 255 || rank < 0 || rank >= world) return r.refuse("bad window shard %d/%d", rank, world);
  // the single-launch kernel; with "glv" (the caller vouches for G1) over the 2n entries of the endomorphism split when they fit
  if (sw.small_msm && world == 1) {
    const bool sglv = sw.glv && 2 * n <= SM_MAX_N && small_fits_one(2 * n, c, true);
    if (sglv || small_fits_one(n, c, false)) {
      r.engine = ENGINE_SMALL; r.glv = sglv; r.c = c ? c : pick_small_c(sglv ? 2 * n : n);
      r.plan = make_plan(r.c, sglv);
      return r;
    }
  }
  // the endomorphism split ("glv": the caller vouches that the points lie in G1): 2n records, half the windows.  Not for resident
  // vectors (their tables hold n records) nor beyond the partition sort's 2^23 entries per window.
  r.glv = src_kind != SRC_PREPARED && sw.use_partition_sort && 2 * n <= PART_MAX_N && (sw.glv == 2 || (sw.glv == 1 && n <= (size_t)sw.glv_max_n));
  if (c == 0) c = pick_plan_c(r.glv ? 2 * n : n, sw.auto_plan);
  const int cabs = c < 0 ? -c : c;
  if (cabs < 4 || cabs > 16) return r.refuse("window width %d out of range [4,16]", c);
  r.c = c; r.plan = make_plan(c, r.glv);
  r.engine = sw.split && n >= sw.split_min_n && win_count(r.plan.nwin, rank, world) >= 2 ? ENGINE_TWO_CHAINS_A : ENGINE_CHAIN_A;
  return r;
}

// The two-chain form's window selectors: of this rank's windows the upper ones on the context, the lower ones on its child.
static void split_selectors(const WinPlan& plan, int rank, int world, int& sel_hi, int& sel_lo) {
  const int n_own = win_count(plan.nwin, rank, world), n_lo = n_own / 2;
  sel_hi = win_sel(world, n_lo, n_own - n_lo); sel_lo = win_sel(world, 0, n_lo);
}

// M independent MSMs over N terms in all, the largest of max_n (cg1_msm_batched_device).  half_empty: the first or the second M / 2 MSMs
// hold no term at all (then one chain).
static Route route_batched_call(const MsmSwitches& sw, size_t M, size_t N, size_t max_n, int c, bool half_empty) {
  Route r;
  if (M == 0 || N == 0) return r;
  if (N >= (1ull << 31) || M > 65535) return r.refuse("batch too large");
  // A handful of small MSMs (the 4 - 6 of a prover's halving round, prover_kernels.py): ONE k_msm_small launch carries them all
  // (grid.z = MSM) and their Horners run side by side on the host -- the regime-B launch chain costs ~0.5 ms whatever it sums.
  const bool sglv = sw.glv && 2 * max_n <= SM_MAX_N;
  const size_t max_nn = sglv ? 2 * max_n : max_n;
  const int cs = c > 0 ? c : pick_small_c(max_nn);
  const size_t groups = M * (size_t)((sglv ? 127 : 255) / cs + 1) * ((max_nn + SM_SLICE - 1) / SM_SLICE);
  if (sw.small_msm && M <= SM_MAX_MSMS && max_nn <= SM_MAX_N && groups <= SM_MAX_GROUPS && cs >= 4 && cs <= 9 && cs != 5) {
    r.engine = ENGINE_SMALL; r.glv = sglv; r.c = cs; r.plan = make_plan(cs, sglv);
    return r;
  }
  // regime B with the endomorphism split ("glv" != 0: the caller vouches for G1): 2N records and entries, half the windows -- half the
  // (MSM, window) groups whose buckets k_seg_reduce / k_group_reduce sum at the lane rate, half the doublings of every MSM's Horner
  r.glv = sw.glv != 0 && 2 * N < (1ull << 31);
  if (c <= 0) c = pick_window_batched((N + M - 1) / M, r.glv);
  if (c < 4 || c > 9) return r.refuse("batched window width %d out of range [4,9]", c);
  r.c = c; r.plan = make_plan(c, r.glv);
  r.engine = sw.batched_split && M >= (size_t)sw.batched_split_min_m && !half_empty ? ENGINE_TWO_CHAINS_B : ENGINE_CHAIN_B;
  return r;
}

// ------------------------------------------------------------------ the reduction tail, as the launch code switches on it
// (each enum's values are its field's codes in Ctx::last_tail, host_context.h)
enum Fold { FOLD_NONE = 0, FOLD_QUAD = 1, FOLD_LANES = 2 };                                    // -, k_bucket_fold_quad, k_bucket_fold
enum Rowcol { ROWCOL_NONE = 0, ROWCOL_QUAD_ROW = 1, ROWCOL_QUAD = 2, ROWCOL_LANES = 3, ROWCOL_SEG = 4 };      // k_rowcol_quad_row, k_rowcol_quad, k_rowcol, k_seg_reduce
enum Tree { TREE_NONE = 0, TREE_ROW = 1, TREE_QUAD = 2, TREE_LANES = 3 };                      // k_small_tree_row, k_small_tree_quad, k_small_tree
enum Export { EXPORT_NONE = 0, EXPORT_TREE = 1, EXPORT_KERNEL = 2, EXPORT_COPY = 3 };          // k_small_tree_row itself, k_export_host, hipMemcpyAsync
enum Horner { HORNER_NONE = 0, HORNER_HOST = 1, HORNER_ROW = 2, HORNER_QUAD = 3, HORNER_LANES = 4 };      // host, k_msm_horner_row, k_msm_horner_quad, k_msm_horner
struct TailPlan {
  Fold fold = FOLD_NONE; Rowcol rowcol = ROWCOL_NONE; Tree tree = TREE_NONE; Export exp = EXPORT_NONE; Horner horner = HORNER_NONE;
  uint32_t lgq = 0, rcquad = 0, seg_m = 0;      // k_rowcol_quad's log2 of the quads per row / column; k_rowcol's use_quad; k_seg_reduce's segment length
  uint32_t tree_block = 0, nth = 0;             // threads of the tree kernel's block; threads of the host Horner (0: the process's worker pool)
  uint32_t small = 0;                           // k_msm_small: 1 with row_tail = 0, 2 with row_tail = 1
};
static uint32_t tail_word(const TailPlan& t) {
  return ((uint32_t)t.fold << TAIL_FOLD) | ((uint32_t)t.rowcol << TAIL_ROWCOL) | (t.lgq << TAIL_LGQ) | (t.rcquad << TAIL_RCQUAD) | (t.seg_m << TAIL_SEGM) |
         ((uint32_t)t.tree << TAIL_TREE) | ((t.tree_block >> 6) << TAIL_WAVES) | ((uint32_t)t.exp << TAIL_EXPORT) | ((uint32_t)t.horner << TAIL_HORNER) |
         (t.nth << TAIL_NTH) | (t.small << TAIL_SMALL);
}
// a tail word with its Horner fields replaced (the host Horner's thread count is known only once the exported points are)
static uint32_t tail_with_horner(uint32_t word, Horner h, uint32_t nth) {
  return (word & ~((7u << TAIL_HORNER) | (7u << TAIL_NTH))) | ((uint32_t)h << TAIL_HORNER) | (nth << TAIL_NTH);
}
// threads of regime A's host Horner when the highest exported point that is not the identity has weight 2^e_top
static int host_horner_threads(const MsmSwitches& sw, int e_top) {
  return (!sw.host_split || e_top < 96) ? 1 : (sw.horner_threads >= 4 && e_top >= 112 ? 4 : 2);      // (112: the 128-position plans of the endomorphism split)
}
// k_msm_small's word: its own tail, the Horner on the host -- msm_finish's for one MSM, one thread per MSM for up to four, the worker pool beyond
static TailPlan small_tail(const MsmSwitches& sw) { TailPlan t; t.small = sw.small_row_tail ? 2u : 1u; return t; }
static uint32_t small_horner_threads(const MsmSwitches& sw, size_t M, int e_top) { return M == 1 ? (uint32_t)host_horner_threads(sw, e_top) : (M <= 4 ? (uint32_t)M : 0u); }

// ------------------------------------------------------------------ the chunk length of a call
// Grows with the total entry count so that k_accumulate keeps >= 2^18 lanes busy without flooding the
// reduce phases with chunk sums (64 at 2^20 terms x 16 windows, 512 at 2^23) and shrinks to the minimum (8) for
// small inputs, where the dependent madd chain of one chunk IS the critical path.  Buckets cut into several chunks
// (window-sharded ranks, skew, thin top windows) are re-joined by k_bucket_fold (<= 16 chunks) / k_heavy_combine.
static uint32_t grown_chunk_len(uint32_t L0, uint64_t entries) {
  while (L0 < 65536u && (entries >> 18) > (uint64_t)L0) L0 <<= 1;
  return L0;
}

// ------------------------------------------------------------------ regime A: everything msm_enqueue derives
struct ChainPlan {
  WinPlan plan; int rank = 0, world = 1;                  // `world` is a window selector (kernels_prepare_digits.h win_sel): the share w = rank (mod world), or a run of it
  bool resident = false;                                  // the points are prepared records already (a cg1_vec, or the other chain's)
  size_t n_real = 0, n = 0;                               // terms; digit rows = records (an endomorphism-split call runs over 2n records -- P_i, then phi(P_i))
  int nlw = 0, nbits = 0;                                 // windows this chain owns (<= 0: nothing to launch); bits of the segment index
  uint32_t NB = 0, m = 0, J = 0;                          // buckets per window; segment length and segments per window of the 1-D form
  uint32_t bb = 0, lb2 = 0, hb2 = 0;                      // 2-D split of the bucket index
  bool use2d = true; uint32_t nitems = 0; size_t nb_total = 0;
  uint32_t L = 0;                                         // the call's chunk length
  bool partition = true;                                  // two-level partition sort (no global atomics), else the global-atomic counting sort (any n < 2^31)
  uint32_t sub_bits = 0, nbins = 0, nslices = 0, nbc = 0; int big_bins = 0;
  bool uscan_one = false, scan_one = false;               // the partition counts' scan / the bucket scan as one single-block launch
  TailPlan tail;
};
static ChainPlan plan_regime_a(const MsmSwitches& sw, size_t n, const WinPlan& plan, int rank, int world, bool resident) {
  ChainPlan p;
  p.plan = plan; p.rank = rank; p.world = world; p.resident = resident;
  p.n_real = n; p.n = plan.glv ? 2 * n : n;               // everything behind the digit kernel sees an MSM of `n` = 2 n_real points
  n = p.n;
  p.nlw = win_count(plan.nwin, rank, world);
  if (p.nlw <= 0) return p;
  p.bb = (uint32_t)plan.cmax - 1u; p.lb2 = (p.bb + 1u) / 2u; p.hb2 = p.bb - p.lb2;
  p.NB = 1u << p.bb; p.m = std::min<uint32_t>(sw.seg_m, p.NB); p.J = p.NB / p.m;
  while ((1u << p.nbits) < p.J) ++p.nbits;
  p.use2d = sw.reduce_2d != 0;
  p.nitems = p.use2d ? 1u + p.hb2 + p.lb2 : 1u + (uint32_t)p.nbits;
  p.nb_total = (size_t)p.nlw * p.NB;
  const uint64_t entries = (uint64_t)n * (uint64_t)p.nlw;
  p.L = grown_chunk_len(sw.L0, entries);
  // Between 2^17 and 2^19 terms k_accumulate is already bound by throughput, not by the chain of one chunk, and the lane-per-bucket tail
  // runs (more than 2^18 buckets): there a chunk should hold a WHOLE bucket -- mean load m plus eight standard deviations of its Poisson
  // spread -- so that no bucket is cut, k_bucket_fold finds nothing to do and k_rowcol reads one sum per bucket (profiles/r04_chunk_ab.txt:
  // 2^18 terms 1.22 -> 1.11 ms).  Below 2^22 entries the chain still shows: 20 at most (2^17 terms: 0.94 -> 0.91 ms).
  if (sw.chunk_rule && world == 1) {
    if (entries >= (1ull << 20) && entries < (1ull << 21) && p.L < 10u) p.L = 10u;      // 2^16 terms: 0.715 -> 0.695 ms (same file)
    if (entries >= (1ull << 21) && entries < (1ull << 24) && p.nb_total > (size_t)sw.rowcol_quad_max) {
      const double mload = (double)n / (double)(1u << p.bb);
      uint32_t want = (uint32_t)(mload + 8.0 * std::sqrt(mload) + 1.0);
      if (entries < (1ull << 22) && want > 20u) want = 20u;
      if (want > p.L) p.L = want;
    }
  }
  p.partition = sw.use_partition_sort && n <= PART_MAX_N;
  if (p.partition) {
    // bins per window = 2^(bb - sub_bits) <= 128 (the partition kernels' LDS tables); a bin is ONE workgroup of k_bin_sort, so mid sizes
    // want many small bins ("sort_sub_bits": the sub-bucket width, 8 at most; A/B in profiles/r04_sort_bins_ab.txt)
    const uint32_t want_sub = sw.sort_sub_bits ? (uint32_t)sw.sort_sub_bits : (n <= ((size_t)1 << 16) ? 7u : 8u);   // 0 = by size: measured
    p.sub_bits = p.bb < want_sub ? p.bb : want_sub;
    while (p.bb - p.sub_bits > 7u) ++p.sub_bits;
    p.nbins = 1u << (p.bb - p.sub_bits);
    p.nslices = ((uint32_t)n + PART_TILE - 1) / PART_TILE;
    p.nbc = (uint32_t)p.nlw * p.nbins * p.nslices;
    p.uscan_one = sw.scan_one && p.nbc <= USCAN1_MAX;
    p.scan_one = sw.scan_one && p.nb_total <= SCAN1_MAX;
    // the slice path for bins beyond k_bin_sort's LDS stage: a bin cannot exceed n entries, and up to twice the stage k_bin_sort's
    // direct path is as fast as three more launches even for all-equal scalars (2^14 terms: 0.766 -> 0.752 ms, uniform 0.409 -> 0.401)
    p.big_bins = sw.big_bins && (uint32_t)n > 2u * BIN_STAGE;
  }
  TailPlan& t = p.tail;
  // k_rowcol_quad (every addition by a DPP quad) only where the reduction is a pure latency chain: a few thousand buckets
  const bool small_quad = sw.quad && sw.rowcol_quad && p.nb_total <= (size_t)sw.rowcol_quad_max;
  const bool row_pair = sw.rowcol_row && sw.tree_row;      // one wave per row / column, the cross-quad levels on rows (its sums are in row form: k_small_tree_row reads them)
  // Buckets cut into 2..16 chunks are folded into their first slot before the row / column sums (k_rowcol_quad requires it, so with it
  // as the consumer a fold is launched whatever "fold_quad" and "fold_pass" say;
  // k_rowcol / k_seg_reduce could add the chunk sums themselves -- bucket_sum -- but the divergent trip counts inside their lanes
  // cost more than the separate pass: profiles/r03_rowcol_ab.txt).
  // k_rowcol_quad_row can add a bucket's chunk sums itself: worth it only for a few thousand buckets (2^12 terms 0.354 -> 0.336 ms; at 2^15 -
  // 2^16 the uneven trip counts of a wave's quads cost more than the separate pass: 0.605 -> 0.657, profiles/r05_tree_row_ab.txt)
  const bool rows_fold = small_quad && p.use2d && row_pair && p.nb_total <= 8192;
  if (rows_fold) t.fold = FOLD_NONE;
  else if (small_quad && sw.fold_quad) t.fold = FOLD_QUAD;
  else if (sw.fold_pass || (small_quad && p.use2d && !row_pair)) t.fold = FOLD_LANES;      // (k_rowcol_quad has no bucket_sum loop: "fold_pass" = 0 cannot apply to it)
  const bool zc = sw.zero_copy != 0;
  if (!p.use2d) {
    t.rowcol = ROWCOL_SEG; t.seg_m = p.m;
    t.exp = zc ? EXPORT_KERNEL : EXPORT_COPY;
    return p;
  }
  const uint32_t R = 1u << p.hb2, Cn = 1u << p.lb2;
  if (small_quad && row_pair) t.rowcol = ROWCOL_QUAD_ROW;
  else if (small_quad) {
    // quads per row / column: 16, 8 or 4 (a wave carries 1, 2 or 4 rows).  Measured (profiles/r04_rowcol_ab.txt, fold + row / column
    // sums at 2^12 .. 2^16 terms): a serial element costs a quad ~8 us, a shuffle level ~23 us (56 words through ds_bpermute), and
    // 2 560 one-wave rows are 1.25 rounds of the 2 048 resident waves -- so FEW quads per row win: 4 where rows and columns are equally
    // long (119 / 104 / 97 us at 2^12, 248 / 229 / 216 at 2^16 for 16 / 8 / 4 quads), 8 where they are not (2^14: 158 / 150 / 167).
    t.rowcol = ROWCOL_QUAD;
    t.lgq = sw.rowcol_lgq >= 2 && sw.rowcol_lgq <= 4 ? (uint32_t)sw.rowcol_lgq : (R == Cn ? 2u : 3u);
  } else { t.rowcol = ROWCOL_LANES; t.rcquad = sw.quad ? 1u : 0u; }
  if (sw.tree_row) {
    uint32_t W = (1u << std::max(p.hb2, p.lb2)) >> 3;      // ~8 selected elements per wave at most, 16 waves at most
    t.tree = TREE_ROW; t.tree_block = 64u * (W < 1u ? 1u : (W > 16u ? 16u : W));
  } else if (sw.quad) {
    // 4 lanes per element of the longer of the two sums (2^hb rows, 2^lb columns), at most 512 threads: no idle quads in the block
    const uint32_t tree_threads = std::min<uint32_t>(512u, std::max<uint32_t>(64u, 4u << std::max(p.hb2, p.lb2)) >> (sw.tree_shift >= 0 ? sw.tree_shift : (sw.tree_half ? 1 : 0)));
    t.tree = TREE_QUAD; t.tree_block = std::max<uint32_t>(64u, tree_threads);
  } else { t.tree = TREE_LANES; t.tree_block = 256u; }
  // zero-copy calls: from k_small_tree_row the items, the status words and the flag word go to the mapped host records (no k_export_host)
  t.exp = !zc ? EXPORT_COPY : (t.tree == TREE_ROW ? EXPORT_TREE : EXPORT_KERNEL);
  return p;
}

// ------------------------------------------------------------------ regime B: everything batched_chain_enqueue derives
struct BatchPlan {
  int rc = CG1_OK;                       // CG1_ERR_ARG: "batch too large"
  WinPlan plan; int c = 0; uint32_t nwin = 0, NB = 0, m = 0, log2m = 0, J = 0, L = 0;
  size_t G = 0, nb_total = 0, Nv = 0;    // (MSM, window) groups; buckets; entries per digit row = prepared records
  bool host_horner = false;
  TailPlan tail;
};
static BatchPlan plan_regime_b(const MsmSwitches& sw, size_t M, size_t N, int c, bool glv) {
  BatchPlan p;
  p.plan = make_plan(c, glv); p.c = c;
  p.nwin = (uint32_t)p.plan.nwin; p.NB = 1u << (c - 1);
  p.G = M * p.nwin; p.nb_total = p.G * p.NB;
  p.Nv = glv ? 2 * N : N;
  if (p.nb_total >= (1ull << 31) || p.Nv * p.nwin >= (1ull << 31)) { p.rc = CG1_ERR_ARG; return p; }
  p.m = 8 < p.NB ? 8 : p.NB;             // segment length of k_seg_reduce
  while ((1u << p.log2m) < p.m) ++p.log2m;
  p.J = p.NB / p.m;
  p.L = grown_chunk_len(sw.L0, (uint64_t)p.Nv * (uint64_t)p.nwin);
  // The Horner over an MSM's window sums is 255 DEPENDENT doublings: ~1.0 ms for a DPP quad, ~65 us for a host core.  A handful of
  // MSMs (the prover's halving rounds: 4-6 per call) therefore finish on the host, on the context's four threads; hundreds of them
  // (a batch of accumulator MSMs) keep the device's one-quad-per-MSM kernel, which does them all in the same millisecond.
  p.host_horner = M <= (size_t)sw.batched_host_horner_max;
  TailPlan& t = p.tail;
  t.rowcol = ROWCOL_SEG; t.seg_m = p.m; t.exp = EXPORT_COPY;
  if (p.host_horner) { t.horner = HORNER_HOST; t.nth = (uint32_t)std::min<size_t>(4, M); }      // (batched_chain_finish: up to four host threads)
  // up to ~2 000 MSMs one WAVE each, one limb per lane (fp_row.h: a lone wave's doubling in ~1.5 us instead of a quad's ~5); beyond,
  // a wave per MSM would be eight and more to a SIMD and the quads' throughput wins (profiles/r05_rowlane_ab.txt)
  else t.horner = sw.horner_row && M <= 2048 ? HORNER_ROW : (sw.quad ? HORNER_QUAD : HORNER_LANES);
  return p;
}

}  // namespace cg1
