// Host side of the MSM engine, part 1: the per-device context (streams, helper threads, scratch buffers and their growth).
// Part of the single translation unit csrc/msm_gpu.hip (included there, in this order; not a stand-alone header).
#pragma once

namespace cg1 {

// ------------------------------------------------------------------ host-side context
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
  snprintf(ctx->err, sizeof ctx->err, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); return CG1_ERR_HIP; } } while (0)

// One persistent helper thread per context for the second half of the host Horner tail (a std::async per call paid a
// thread creation, ~40 us, on a ~150 us tail).
struct Helper {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<void()> job;
  bool has = false, done = true, quit = false, armed = false;
  std::atomic<bool> posted{false};       // mirrors `has` for a helper that is spinning (arm())
  std::atomic<bool> stand_down{false};   // disarm(): the spinning helper gives up at once
  void start_locked() { if (!th.joinable()) th = std::thread([this]() { loop(); }); }
  void run(std::function<void()> f) {
    std::unique_lock<std::mutex> lk(mu);
    start_locked();
    job = std::move(f); has = true; done = false;
    posted.store(true, std::memory_order_release);
    cv.notify_all();
  }
  // A job is about to come (the caller starts polling for a GPU result a fraction of a millisecond away): wake the thread now and
  // let it SPIN for the job (at most ~2 ms) instead of paying the futex wake-up -- 20-40 us -- inside a 100 us host tail.
  void arm() {
    std::unique_lock<std::mutex> lk(mu);
    start_locked();
    if (!has && done) { stand_down.store(false, std::memory_order_relaxed); armed = true; cv.notify_all(); }
  }
  // no job will come after all (the call failed, or its tail needs fewer threads than were armed): stop spinning, go back to sleep
  void disarm() { stand_down.store(true, std::memory_order_release); }
  void wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this]() { return done; });
  }
  void loop() {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [this]() { return has || quit || armed; });
      if (quit) return;
      if (!has) {                                              // armed: spin for the job outside the lock
        armed = false;
        lk.unlock();
        const auto until = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
        for (uint32_t k = 0; !posted.load(std::memory_order_acquire); ++k) {
          if (stand_down.load(std::memory_order_acquire)) break;
          if ((k & 0xffu) == 0xffu && std::chrono::steady_clock::now() > until) break;
          __builtin_ia32_pause();
        }
        lk.lock();
        if (!has) continue;
      }
      armed = false;
      std::function<void()> f = std::move(job);
      has = false;
      posted.store(false, std::memory_order_relaxed);
      lk.unlock();
      f();
      lk.lock();
      done = true;
      cv.notify_all();
    }
  }
  ~Helper() {
    { std::unique_lock<std::mutex> lk(mu); quit = true; cv.notify_all(); }
    if (th.joinable()) th.join();
  }
};

// Every switch the MSM launch chains and their planner (msm_plan.h) read, with its default.  A context IS one (Ctx derives from it), so a
// second launch chain's context takes them all with one assignment, and the planner can be asked about a call without a context.
struct MsmSwitches {
  uint32_t L0 = 8;                      // "chunk_len": MINIMUM chunk length; the per-call length grows with the entry count
  uint32_t seg_m = 4;                   // "seg_m": segment length of k_seg_reduce (1, 2, 4, 8, 16)
  int chunk_rule = 1;                   // "chunk_rule": whole-bucket chunks at 2^17 .. 2^19 terms (A/B switch)
  int stage_sort = 1;                   // LDS-staged, line-coalesced writes in k_part_scatter / k_bin_sort (A/B switch)
  int quad = 1;                         // quad-lane EC ops in the latency-bound kernels (A/B switch)
  int reduce_2d = 1;                    // 1: k_rowcol + k_small_tree; 0: k_seg_reduce + k_bit_tree (A/B switch)
  int use_partition_sort = 1;           // "partition_sort": the two-level LDS partition sort up to 2^23 rows; 0: the global-atomic counting sort
  int big_bins = 1;                     // giant bins of skewed scalars sorted by many blocks (A/B switch)
  int sort_sub_bits = 0;                // partition sort: sub-bucket bits a k_bin_sort workgroup sorts by ("sort_sub_bits": 4 .. 8; 0 = 7 up to 2^16 terms, else 8)
  int scan_one = 1;                     // the sort's two scans as one single-block launch each when they are small (A/B switch)
  int fold_pass = 1;                    // k_bucket_fold in front of k_rowcol / k_seg_reduce; 0 leaves multi-chunk buckets to their bucket_sum loops
                                        // (measured WORSE: 372 instead of 235 us at 2^16 -- divergent trip counts inside the row / column lanes)
  int fold_quad = 1;                    // "fold_quad": small bucket counts: k_bucket_fold_quad (1) or the one-lane-per-bucket k_bucket_fold (0); A/B switch
  int rowcol_quad = 1;                  // k_rowcol_quad for small bucket counts (A/B switch)
  int rowcol_quad_max = 1 << 18;        // ... up to this many buckets ("rowcol_quad_max")
  int rowcol_lgq = 0;                   // "rowcol_lgq": log2 of the quads per row / column of k_rowcol_quad (2, 3, 4; 0 = by cost)
  int rowcol_row = 1;                   // "rowcol_row": with tree_row, small bucket counts: k_rowcol_quad_row (one wave per row / column, the cross-quad levels on rows)
  int tree_row = 1;                     // "tree_row": regime A's 1 + hb + lb items per window by blocks of waves with one limb per lane (k_small_tree_row); 0: k_small_tree_quad
  int tree_shift = 2;                   // "tree_shift": k_small_tree_quad's block = 4 lanes per element >> this (0 .. 4; -1 = tree_half's 0 / 1).  Measured
                                        // (profiles/r04_tree_ab.txt, tree + export at 2^16 / 2^18 / 2^20): 0: 111 / 112 / 119 us, 1: 90 / 112 / 121, 2: 79 / 100 / 110, 4: 78 / 161 / 177
  int tree_half = 1;                    // k_small_tree_quad: 2 lanes per element (a quad takes two elements) instead of 4 (A/B switch)
  int zero_copy = 1;                    // 1: export kernel + flag polling instead of a D2H copy + stream wait (A/B switch)
  int host_split = 1;                   // host Horner tail on two threads (A/B switch)
  int arm_helpers = 1;                  // "arm_helpers": the Horner's helper threads spin for their part while a small / mid-size call's result is polled (A/B switch)
  int horner_threads = 4;               // host threads of the Horner tail: 1, 2 or 4 (A/B switch; host_split = 0 forces 1)
  int horner_row = 1;                   // "horner_row": regime B's device Horner with one wave per MSM, one limb per lane (A/B switch; 0: one quad per MSM)
  int batched_host_horner_max = 24;     // regime B calls with at most this many MSMs run their Horner on the host ("batched_host_horner_max")
  int small_msm = 1;                    // "small_msm": MSMs of <= SM_MAX_N = 2048 terms as ONE launch (k_msm_small); 0 = the regime-A chain (A/B switch)
  int small_row_tail = 1;               // "small_row_tail": k_msm_small's items / combine / export one limb per lane, one wave per item (A/B switch)
  int glv = 0;                          // "glv": the caller vouches that every point of its MSM calls lies in the prime-order subgroup, and the engine may run
                                        // the endomorphism split (csrc/glv.h): 1 = where it pays (the single-launch kernel up to 1 024 terms, regime A up to
                                        // glv_max_n terms), 2 = wherever it can (A/B runs).  WRONG results outside G1: default 0.
  int glv_max_n = 1 << 14;              // "glv_max_n": largest regime-A call glv = 1 splits (profiles/r05_glv_ab.txt: slower from 2^15 terms up)
  int auto_plan = 1;                    // window_c = 0 picks balanced window plans for mid-size inputs (A/B switch)
  // "split" (A/B switch, OFF): one large call as TWO launch chains on two streams -- the high half of the windows on this context, the
  // low half on `child` (own scratch buffers, stream and export flag; shared prepared points) -- meant to run the low half's sort under
  // the high half's k_accumulate and the high half's reduction tail under the low half's.  MEASURED A LOSS (profiles/r04_split_ab.txt:
  // 2^20 3.25 ms against 2.95, 2^18 1.54 against 1.22; only 2^16 gains 3 %): the resident blocks of k_accumulate hold every SIMD's
  // registers for their whole ~1 ms life, so the other stream's kernels are dispatched only when it drains -- the two chains run one
  // after the other, and each pays its own launch chain and the shorter chunks of half the entries.
  int split = 0;
  size_t split_min_n = (size_t)1 << 17; // "split_min_log2n": ... from this many terms on
  int batched_split = 0;                // "batched_split": regime B as two launch chains of half the MSMs each, the second half's k_accumulate behind the first's
                                        // (so that the first half's tail runs under it).  Measured SLOWER (1 024 x 627: 5.2-5.3 -> 5.6-5.8 ms, with the
                                        // endomorphism split 4.72 -> 4.76-4.85, profiles/r05_regime_b_split.txt): the tails are not idle time.  A/B switch, off.
  int batched_split_min_m = 256;        // "batched_split_min_m": ... from this many MSMs on
  int blocking_sync = 0;                // waits sleep on an interrupt (Ctx::sync_ev) instead of spinning a core
  int profile = 1;                      // 0: no hipEvents; 1: around k_accumulate only; 2: around every phase (read_phase_events)
};

// cg1_ctx_set_param's MSM names with their ranges, on a bare switch set (cg1_msm_call_describe applies its inputs through it too).
enum { SW_SET = 0, SW_RANGE = 1, SW_UNKNOWN = 2 };
static int set_msm_switch(MsmSwitches& sw, const char* name, int value) {
  struct Named { const char* name; int MsmSwitches::* field; int lo, hi; };        // lo > hi: any value, stored as 0 / 1
  static const Named table[] = {
    {"chunk_rule", &MsmSwitches::chunk_rule, 1, 0}, {"stage_sort", &MsmSwitches::stage_sort, 1, 0}, {"quad", &MsmSwitches::quad, 1, 0},
    {"reduce_2d", &MsmSwitches::reduce_2d, 1, 0}, {"partition_sort", &MsmSwitches::use_partition_sort, 1, 0}, {"big_bins", &MsmSwitches::big_bins, 1, 0},
    {"scan_one", &MsmSwitches::scan_one, 1, 0}, {"fold_pass", &MsmSwitches::fold_pass, 1, 0}, {"fold_quad", &MsmSwitches::fold_quad, 1, 0},
    {"rowcol_quad", &MsmSwitches::rowcol_quad, 1, 0}, {"rowcol_quad_max", &MsmSwitches::rowcol_quad_max, 0, INT32_MAX}, {"rowcol_row", &MsmSwitches::rowcol_row, 1, 0},
    {"tree_row", &MsmSwitches::tree_row, 1, 0}, {"tree_shift", &MsmSwitches::tree_shift, -1, 4}, {"tree_half", &MsmSwitches::tree_half, 1, 0},
    {"zero_copy", &MsmSwitches::zero_copy, 1, 0}, {"host_split", &MsmSwitches::host_split, 1, 0}, {"arm_helpers", &MsmSwitches::arm_helpers, 1, 0},
    {"horner_row", &MsmSwitches::horner_row, 1, 0}, {"batched_host_horner_max", &MsmSwitches::batched_host_horner_max, 0, INT32_MAX},
    {"small_msm", &MsmSwitches::small_msm, 1, 0}, {"small_row_tail", &MsmSwitches::small_row_tail, 1, 0}, {"glv", &MsmSwitches::glv, 0, 2},
    {"glv_max_n", &MsmSwitches::glv_max_n, 0, INT32_MAX}, {"auto_plan", &MsmSwitches::auto_plan, 1, 0}, {"split", &MsmSwitches::split, 1, 0},
    {"batched_split", &MsmSwitches::batched_split, 1, 0}, {"batched_split_min_m", &MsmSwitches::batched_split_min_m, 2, INT32_MAX},
    {"blocking_sync", &MsmSwitches::blocking_sync, 1, 0}, {"profile", &MsmSwitches::profile, 0, 2},
  };
  for (const Named& t : table) {
    if (strcmp(name, t.name)) continue;
    if (t.lo <= t.hi && (value < t.lo || value > t.hi)) return SW_RANGE;
    sw.*t.field = t.lo <= t.hi ? value : (value ? 1 : 0);
    return SW_SET;
  }
  // the names whose values are not a plain interval, or not an int field
  const auto one_of = [value](std::initializer_list<int> ok) { return std::find(ok.begin(), ok.end(), value) != ok.end(); };
  if (!strcmp(name, "chunk_len")) { if (value < 1 || value > 65536) return SW_RANGE; sw.L0 = (uint32_t)value; return SW_SET; }
  if (!strcmp(name, "seg_m")) { if (!one_of({1, 2, 4, 8, 16})) return SW_RANGE; sw.seg_m = (uint32_t)value; return SW_SET; }
  if (!strcmp(name, "horner_threads")) { if (!one_of({1, 2, 4})) return SW_RANGE; sw.horner_threads = value; return SW_SET; }
  if (!strcmp(name, "rowcol_lgq")) { if (!one_of({0, 2, 3, 4})) return SW_RANGE; sw.rowcol_lgq = value; return SW_SET; }
  if (!strcmp(name, "sort_sub_bits")) { if (!one_of({0, 4, 5, 6, 7, 8})) return SW_RANGE; sw.sort_sub_bits = value; return SW_SET; }
  if (!strcmp(name, "split_min_log2n")) { if (value < 10 || value > 31) return SW_RANGE; sw.split_min_n = (size_t)1 << value; return SW_SET; }
  return SW_UNKNOWN;
}

struct Ctx : MsmSwitches {
  int device = 0;
  Helper helper[3];                     // the host Horner tail runs on up to four threads (this one + three helpers)
  hipStream_t stream = nullptr;
  std::atomic<hipStream_t> copy_stream{nullptr};    // H2D staging copies that overlap kernels on `stream` (cg1_h2d_async / cg1_copy_fence); created at the first
  std::once_flag copy_once;              // such copy: a context that never stages (the verifier's front-end lanes) holds ONE stream -- a process
                                        // has 24 hardware queues, and streams that share one run one after the other
  hipEvent_t copy_ev = nullptr;
  std::vector<uint32_t> cu_mask;        // non-empty: the compute and side streams are confined to these CUs
  hipStream_t side_stream = nullptr;    // small latency-bound kernels that run BESIDE the compute stream (cg1_subgroup_flags_enqueue)
  hipEvent_t side_ev = nullptr;
  hipEvent_t sync_ev = nullptr;         // blocking-sync event: waits sleep on an interrupt instead of spinning a core
  char err[256] = {0};
  int alloc_fail_at = 0;                // "alloc_fail_at": the k-th allocation grow_bufs attempts from now on fails as out of memory (a test's hook; 0 = off)
  // capacity
  size_t cap_n = 0, cap_nb = 0, cap_chunks = 0, cap_entries = 0, cap_out = 0;
  PreparedPoint* d_pts = nullptr;
  uint8_t* d_flags = nullptr;
  uint32_t *d_hist = nullptr, *d_off = nullptr, *d_choff = nullptr, *d_sorted = nullptr;
  uint2 *d_blocktot = nullptr, *d_desc = nullptr;
  uint32_t *d_order = nullptr, *d_lenhist = nullptr;      // [2*LEN_BINS]: histogram, cursor  (points into d_zblock)
  // one block cleared by ONE memset per call: chunk-length histogram | any_multi flag | combined[] bytes | heavy count (+ ids)
  uint32_t* d_zblock = nullptr; size_t cap_zblock = 0;
  uint32_t* d_any_multi = nullptr;
  PointSum* d_partial = nullptr; size_t cap_partial = 0;
  uint16_t* d_digits = nullptr; uint32_t* d_part = nullptr; uint32_t* d_blockcnt = nullptr; uint32_t* d_ublocktot = nullptr;
  size_t cap_digits = 0, cap_part = 0, cap_blockcnt = 0;
  uint32_t *d_slice_base = nullptr, *d_slicehist = nullptr, *d_subbase = nullptr; uint8_t* d_bigflag = nullptr;
  size_t cap_bigflag = 0, cap_slices = 0;
  int merlin_sync = 1;                  // k_merlin_batch_sync (lanes permute together) instead of k_merlin_batch (A/B switch)
  uint32_t merlin_clk[2] = {0, 0};
  int fe_timed = 0;                     // "fe_timed": the block-program kernel reads the shader clock around the parts of a pass (cg1_shuffle_fe_last_split)
  int fe_rows = 1;                      // "fe_rows": 1 = the front-end's block-program kernel (k_shuffle_front_end_rows), 0 = the byte machine
  int fe_prio = 0;                      // "fe_prio": wave priority of k_shuffle_front_end (s_setprio 0 .. 3)
  int decompress_waves = 3;             // "decompress_waves": waves per SIMD k_batch_decompress<false> is compiled for (2: table in registers, 3: half of it in scratch)
  void* d_opening = nullptr; size_t cap_opening = 0;              // cg1_opening_prepare_device's scratch (940 B per proof)
  void* d_tscan_tab = nullptr; size_t cap_tscan_tab = 0;          // cg1_tracker_match_device's tile of light-table records (public points only)
  // cg1_exact_relations_device's term records and cg1_exact_gather_device's indices: two page-locked staging blocks with their device copies,
  // used in turn, each with the event recorded behind its last upload (a call waits only for the upload made two calls before it)
  uint8_t *h_exact[2] = {nullptr, nullptr}, *d_exact[2] = {nullptr, nullptr}; size_t cap_exact[2] = {0, 0};
  hipEvent_t exact_ev[2] = {nullptr, nullptr}; int exact_turn = 0;
  int tscan_ladder_max_ks = CG1_TRACKER_MATCH_LADDER_MAX_KS;      // "tracker_scan_ladder_max_ks": up to this many secrets a scan runs one ladder per pair (0: always the tables)
  int tscan_timing = 0; float tscan_ms[2] = {0.f, 0.f};           // "tracker_scan_timing": wait between the phases of a scan and keep build / match wall ms
  void* d_prover = nullptr; size_t cap_prover = 0;                // cg1_opening_prove_device's scratch (1 252 B per proof)
  void* d_register = nullptr; size_t cap_register = 0;            // cg1_whisk_register_device's scratch (capi_register.h): a slice's columns and k_register_points' parking; the secret columns zeroed before every return
  void* d_whisk_draws = nullptr; size_t cap_whisk_draws = 0;      // the seeded draws of Whisk shuffles (capi_whisk_shuffle.h): swaps | perm | scalars; zeroed before every return
  int whisk_resident = 0;               // "whisk_resident_witness": cg1_whisk_shuffle_prove_seeded keeps its draws on the device (k_whisk_witness_place) instead of staging them through the host
  uint64_t whisk_traffic[2] = {0, 0};   // since the last seeded call began: witness bytes copied device -> host | written into host memory by the library (plain host counters beside those sites; cg1_whisk_last_witness_traffic)
  void* d_chain_prove = nullptr; size_t cap_chain_prove = 0;      // the tracker stage of a proved chain (capi_chain_prove.h): certification, origins, composites (zeroed before every return), records
  PreparedPoint* d_gen_tab = nullptr;   // k_generator_mul's table of G (GEN_ENTRIES records), built at the first use (cg1_generator_mul_device)
  int fixed_slice = 0;                  // "fixed_slice": terms per workgroup of k_table_msm (1 .. 128; 0 = by the size of the call).  A/B switch
  int fixed_waves = 0;                  // "fixed_waves": waves per workgroup of k_table_msm (4, 8, 16; 0 = by the size of the call).  A/B switch
  int ipa_inv = 0;                      // "ipa_inv": how k_ipa_step inverts a round challenge (0: binary Euclid, 1: a^(r-2)).  A/B switch
  int merlin_last_kernel = 0;           // which kernel served the last cg1_merlin_batch_device call: 2 block program, 1 byte machine, 0 one lane at a time
  int merlin_rows = 1;                  // "merlin_rows": 1 = cg1_merlin_batch_device hashes whole rate blocks (k_merlin_batch_rows) when the program fits, 0 = byte machine
  void* d_merlin_rows = nullptr; size_t merlin_rows_cap = 0;      // the rows of the last such call (kept: 134 KB per shuffle-shaped transcript)
  int merlin_lanes = 64;                // transcripts per wave of k_merlin_batch_sync ("merlin_lanes": 1 .. 64)
  uint32_t merlin_passes = 0;           // of the last cg1_merlin_batch_device call: Keccak passes of the slowest wave
  int batch_mul_host_max = -1;          // cg1_batch_mul_add (host pointers): outputs up to which the host's pool does the work ("batch_mul_host_max"; -1 = 16 per pool thread, 0 = never)
  int last_batch_mul_on_host = 0;
  int batch_mul_quad_max = 8192;        // k_batch_mul_quad up to this many outputs ("batch_mul_quad_max"; 0 = always one lane per output)
  struct Pending {                      // what msm_finish needs from msm_enqueue
    bool active = false;
    int c = 0, rank = 0, world = 1, nlw = 0, nbits = 0;
    WinPlan plan;
    uint32_t m = 1, lb2 = 0, hb2 = 0, nitems = 0;
    bool use2d = true;
    int profile = 0;                    // the level the events of THIS call were recorded under (may change before msm_finish)
    bool zero_copy = false; uint32_t seq = 0;
    bool arm_helpers = false;           // the host tail is a large share of this call: its helper threads spin for their part while the GPU result is polled
    size_t nout_words = 0;
    const PointWords* hout = nullptr;   // where the exported items land (ctx->h_out, or h_small_out for k_msm_small)
    std::chrono::steady_clock::time_point h0, h1;
  } pend;
  cg1_ctx* child = nullptr;
  hipEvent_t ev_prep = nullptr, ev_acc = nullptr;
  bool pend_split = false;
  int last_acc_launches = 0;            // k_accumulate launches of the last MSM call: 2 (split), 1, or 0 (k_msm_small)
  PointSum* d_small_partial = nullptr; size_t cap_small_partial = 0;
  uint32_t* d_small_ctr = nullptr;
  PreparedPoint* d_small_pts = nullptr; uint8_t* d_small_flags = nullptr; size_t cap_small_pts = 0;      // k_prepare_blobs<true> output for un-normalised blob input
  PointWords* h_small_out = nullptr; PointWords* h_small_out_dev = nullptr;     // pinned + mapped: 64 x 9 window items + the status record
  uint32_t* d_heavy = nullptr; size_t cap_heavy = 0;         // [0] count, then heavy bucket ids
  uint8_t* d_combined = nullptr; size_t cap_combined = 0;
  uint32_t* d_boffs = nullptr; size_t cap_boffs = 0;          // regime B: MSM offsets, group sums, per-MSM results
  PointSum* d_gsum = nullptr; size_t cap_gsum = 0;
  PointWords* d_bout = nullptr; PointWords* h_bout = nullptr; size_t cap_bout = 0;
  PointWords* d_gout = nullptr; PointWords* h_gout = nullptr; size_t cap_gout = 0;       // regime B, few MSMs: window sums exported for the host Horner
  int lincomb_zero_copy = 1;            // "lincomb_zero_copy": small GPU shares of cg1_lincomb_batch are read from mapped host memory (no staged copy); A/B switch
  int batch_mul_row = 1;                // "batch_mul_row": deferred map / fold batches of 96 .. 4096 results on k_batch_mul_row (A/B switch; 0: pool / k_batch_mul)
  PointSum *d_sums = nullptr, *d_segrun = nullptr, *d_segtot = nullptr;
  PointWords* d_out = nullptr;
  PointWords* h_out = nullptr;          // pinned, and mapped into the device: k_export_host writes the window sums straight into it
  PointWords* h_out_dev = nullptr;      // the device's address of h_out
  uint32_t* h_flag = nullptr;           // pinned + mapped: k_export_host stores the call's sequence number here when h_out is complete
  uint32_t* h_flag_dev = nullptr;
  uint32_t seq = 0;
  // staging for host-pointer entry points
  void* d_stage_pts = nullptr; void* d_stage_sc = nullptr; size_t cap_stage_pts = 0, cap_stage_sc = 0;      // bytes
  uint8_t* h_lin = nullptr; uint8_t* h_lin_dev = nullptr; size_t cap_h_lin = 0;   // page-locked gather buffer of cg1_lincomb_batch (terms' points | scalars)
  // timing
  hipEvent_t ev[CG1_NPHASE + 1];
  float phase_ms[CG1_NPHASE] = {0};
  float host_tail_ms = 0;
  float host_ms[4] = {0, 0, 0, 0};      // enqueue, wait-for-GPU, event readout, Horner tail
  uint32_t last_chunks = 0, last_entries = 0;   // of the last MSM call: non-zero digits sorted into buckets; chunks k_accumulate ran
  uint32_t last_tail = 0;               // of the last MSM call: which reduction-tail kernels were launched (TAIL_* below; for the tests, cg1_get_last_tail)
  hipEvent_t tm_ev[2] = {nullptr, nullptr};     // cg1_timer_begin / cg1_timer_end
  int last_c = 0, pend_c = 0;
};

// Ctx::last_tail: which leaves of the reduction tail the last call launched, as bit fields.  One word per call, built by tail_word
// (msm_plan.h) from the enums of the call's plan -- the very ones the launch code switches on -- and completed by msm_finish with the host
// Horner's thread count; nothing reads it but cg1_get_last_tail, which exists for the tests (tests/msm_tail_cases.py restates the
// decision and compares; cg1_msm_call_describe gives the same word without a launch).
//   fold    bits 0-1    0 none launched, 1 k_bucket_fold_quad, 2 k_bucket_fold
//   rowcol  bits 2-4    1 k_rowcol_quad_row, 2 k_rowcol_quad, 3 k_rowcol, 4 k_seg_reduce (regime A: + k_bit_tree, k_bit_tree_final; regime B: + k_group_reduce)
//   lgq     bits 5-7    k_rowcol_quad's lgq
//   rcquad  bit 8       k_rowcol's use_quad
//   seg_m   bits 9-13   k_seg_reduce's segment length
//   tree    bits 14-15  1 k_small_tree_row, 2 k_small_tree_quad, 3 k_small_tree
//   waves   bits 16-20  waves of the tree kernel's block
//   export  bits 21-22  1 k_small_tree_row wrote the mapped host records, 2 k_export_host, 3 hipMemcpyAsync
//   horner  bits 23-25  1 host, 2 k_msm_horner_row, 3 k_msm_horner_quad, 4 k_msm_horner
//   nth     bits 26-28  threads of the host Horner (0: the process's worker pool)
//   small   bits 29-30  1 k_msm_small with row_tail = 0, 2 with row_tail = 1
constexpr uint32_t TAIL_FOLD = 0, TAIL_ROWCOL = 2, TAIL_LGQ = 5, TAIL_RCQUAD = 8, TAIL_SEGM = 9, TAIL_TREE = 14, TAIL_WAVES = 16, TAIL_EXPORT = 21,
                   TAIL_HORNER = 23, TAIL_NTH = 26, TAIL_SMALL = 29;

// ------------------------------------------------------------------ kept buffers: one way to grow them, one way to release them
// A buffer a handle keeps between calls: where its pointer lives, the bytes a growth allocates, and for page-locked host memory the
// hipHostMalloc flags and (mapped memory) where the device's address of it goes.
struct KeptBuf {
  void** p; size_t bytes; bool host; unsigned flags; void** dev;
};
template <class T>
static KeptBuf dev_buf(T*& p, size_t bytes = 0) { return {(void**)&p, bytes, false, 0u, nullptr}; }
template <class T>
static KeptBuf host_buf(T*& p, size_t bytes = 0, unsigned flags = hipHostMallocDefault, T** dev = nullptr) { return {(void**)&p, bytes, true, flags, (void**)dev}; }

// Free the buffers of a group: every pointer null (a mapped block's device address too) and, with it, their shared capacity zero.
static void release_bufs(std::initializer_list<KeptBuf> bufs) {
  for (const KeptBuf& b : bufs) {
    if (*b.p) (void)(b.host ? hipHostFree(*b.p) : hipFree(*b.p));
    *b.p = nullptr;
    if (b.dev) *b.dev = nullptr;
  }
}
static void release_bufs(size_t& cap, std::initializer_list<KeptBuf> bufs) { release_bufs(bufs); cap = 0; }

// Regrow a group of buffers that share one capacity, only when it is too small for `need`: all freed, then each allocated at its own
// size, and the capacity becomes `grown` (>= need, in the field's own units: the site's growth policy).  Any failure leaves the whole
// group empty -- pointers null, capacity zero -- so that the next call grows it again instead of running on freed memory, and takes
// the runtime's sticky error with it.  "alloc_fail_at" (cg1_ctx_set_param): the k-th allocation attempted here fails without a call
// into the runtime, down the same path.
static int grow_bufs(Ctx* ctx, size_t& cap, size_t need, size_t grown, std::initializer_list<KeptBuf> bufs) {
  if (need <= cap) return CG1_OK;
  release_bufs(cap, bufs);
  for (const KeptBuf& b : bufs) {
    const bool injected = ctx->alloc_fail_at && --ctx->alloc_fail_at == 0;
    hipError_t e = injected ? hipErrorOutOfMemory : b.host ? hipHostMalloc(b.p, b.bytes, b.flags) : hipMalloc(b.p, b.bytes);
    if (e == hipSuccess && b.dev) e = hipHostGetDevicePointer(b.dev, *b.p, 0);
    if (e == hipSuccess) continue;
    if (!injected) (void)hipGetLastError();
    release_bufs(cap, bufs);
    snprintf(ctx->err, sizeof ctx->err, "growing a kept buffer to %zu bytes failed: %s%s", b.bytes, hipGetErrorString(e), injected ? " (injected: alloc_fail_at)" : "");
    return CG1_ERR_HIP;
  }
  cap = grown;
  return CG1_OK;
}
// ... one device buffer of T ...
template <class T>
static int grow_device(Ctx* ctx, T*& d, size_t& cap, size_t need, size_t grown) { return grow_bufs(ctx, cap, need, grown, {dev_buf(d, grown * sizeof(T))}); }
// ... and a page-locked block with its device twin.  flags: hipHostMalloc's; h_dev (nullable): where a mapped block's device address goes
static int grow_pinned_pair(Ctx* ctx, uint8_t*& h, uint8_t** h_dev, uint8_t*& d, size_t& cap, size_t need, size_t grown, unsigned flags) {
  return grow_bufs(ctx, cap, need, grown, {host_buf(h, grown, flags, h_dev), dev_buf(d, grown)});
}

// the views into d_zblock (none while it is empty): [lenhist 2*LEN_BINS words][any_multi][combined: nb_total bytes][heavy count][heavy ids]
static void zblock_views(Ctx* c, size_t nb_total, size_t hcap) {
  uint32_t* z = c->d_zblock;
  const size_t z0 = 2 * LEN_BINS + 1, h0 = z0 + (nb_total + 3) / 4;
  c->d_lenhist = z;
  c->d_any_multi = z ? z + 2 * LEN_BINS : nullptr;
  c->d_combined = z ? reinterpret_cast<uint8_t*>(z + z0) : nullptr;
  c->d_heavy = z ? z + h0 : nullptr;
  c->cap_heavy = z ? hcap : 0;
  c->cap_combined = z ? nb_total : 0;
}

// the MSM chains' scratch (what ensure() and batched_chain_enqueue grow); the context's other kept buffers go with cg1_ctx_destroy
static void free_bufs(Ctx* c) {
  release_bufs(c->cap_n, {dev_buf(c->d_pts), dev_buf(c->d_flags)});
  release_bufs(c->cap_nb, {dev_buf(c->d_hist), dev_buf(c->d_off), dev_buf(c->d_choff), dev_buf(c->d_blocktot), dev_buf(c->d_segrun), dev_buf(c->d_segtot)});
  release_bufs(c->cap_entries, {dev_buf(c->d_sorted)});
  release_bufs(c->cap_chunks, {dev_buf(c->d_order), dev_buf(c->d_desc), dev_buf(c->d_sums)});
  release_bufs(c->cap_zblock, {dev_buf(c->d_zblock)});
  zblock_views(c, 0, 0);
  release_bufs(c->cap_digits, {dev_buf(c->d_digits)});
  release_bufs(c->cap_part, {dev_buf(c->d_part)});
  release_bufs(c->cap_bigflag, {dev_buf(c->d_bigflag), dev_buf(c->d_slice_base), dev_buf(c->d_subbase)});
  release_bufs(c->cap_slices, {dev_buf(c->d_slicehist)});
  release_bufs(c->cap_blockcnt, {dev_buf(c->d_blockcnt), dev_buf(c->d_ublocktot)});
  release_bufs(c->cap_partial, {dev_buf(c->d_partial)});
  release_bufs(c->cap_out, {dev_buf(c->d_out), host_buf(c->h_out, 0, 0u, &c->h_out_dev)});
  release_bufs(c->cap_boffs, {dev_buf(c->d_boffs)});
  release_bufs(c->cap_gsum, {dev_buf(c->d_gsum)});
  release_bufs(c->cap_bout, {dev_buf(c->d_bout), host_buf(c->h_bout)});
  release_bufs(c->cap_gout, {dev_buf(c->d_gout), host_buf(c->h_gout)});
  release_bufs(c->cap_h_lin, {host_buf(c->h_lin, 0, 0u, &c->h_lin_dev)});
}

static int ensure(Ctx* ctx, size_t n, size_t nb_total, size_t nlw, size_t nitems, uint32_t L, bool need_points = true) {
  size_t entries = n * nlw;
  size_t chunks = nb_total + entries / L + 1;
  int rc = CG1_OK;
  if (need_points && (rc = grow_bufs(ctx, ctx->cap_n, n, n, {dev_buf(ctx->d_pts, n * sizeof(PreparedPoint)), dev_buf(ctx->d_flags, n + 16)}))) return rc;
  if ((rc = grow_bufs(ctx, ctx->cap_nb, nb_total, nb_total,
                      {dev_buf(ctx->d_hist, nb_total * 4), dev_buf(ctx->d_off, (nb_total + 1) * 4), dev_buf(ctx->d_choff, (nb_total + 1) * 4),
                       dev_buf(ctx->d_blocktot, (nb_total / SCAN_ITEMS + 2) * sizeof(uint2)),
                       dev_buf(ctx->d_segrun, nb_total * sizeof(PointSum)),      // >= nb_total / m segments
                       dev_buf(ctx->d_segtot, nb_total * sizeof(PointSum))}))) return rc;
  if ((rc = grow_bufs(ctx, ctx->cap_entries, entries, entries, {dev_buf(ctx->d_sorted, (entries + 1) * 4)}))) return rc;
  if ((rc = grow_bufs(ctx, ctx->cap_chunks, chunks, chunks,
                      {dev_buf(ctx->d_order, chunks * 4), dev_buf(ctx->d_desc, chunks * sizeof(uint2)), dev_buf(ctx->d_sums, chunks * sizeof(PointSum))}))) return rc;
  {
    // the call clears everything up to and including the heavy count with one memset
    const size_t hcap = entries / ((size_t)L * (HEAVY_MIN_CHUNKS - 1)) + 2;     // a heavy bucket holds > (MIN-1)*L entries
    const size_t words = 2 * LEN_BINS + 1 + (nb_total + 3) / 4 + 1 + hcap + 64;     // (+64: room for the 256-byte round-up of the per-call memset)
    rc = grow_bufs(ctx, ctx->cap_zblock, words, words, {dev_buf(ctx->d_zblock, words * 4)});
    zblock_views(ctx, nb_total, hcap);
    if (rc) return rc;
  }
  if (ctx->use_partition_sort && n <= PART_MAX_N) {
    const size_t nslices = (n + PART_TILE - 1) / PART_TILE;
    const size_t nbc = nlw * 128 * nslices + 1;            // nbins <= 128
    const size_t nbins = nlw * 128;
    const size_t max_slices = entries / SLICE + nbins + 1;       // sum over bins of ceil(size / SLICE)
    if ((rc = grow_bufs(ctx, ctx->cap_digits, entries, entries, {dev_buf(ctx->d_digits, entries * 2 + 16)}))) return rc;
    if ((rc = grow_bufs(ctx, ctx->cap_part, entries, entries, {dev_buf(ctx->d_part, (entries + 1) * 4)}))) return rc;
    if ((rc = grow_bufs(ctx, ctx->cap_bigflag, nbins, nbins,
                        {dev_buf(ctx->d_bigflag, nbins + 16), dev_buf(ctx->d_slice_base, (nbins + 1) * 4), dev_buf(ctx->d_subbase, nbins * 256 * 4)}))) return rc;
    if ((rc = grow_bufs(ctx, ctx->cap_slices, max_slices, max_slices, {dev_buf(ctx->d_slicehist, max_slices * 256 * 4)}))) return rc;
    if ((rc = grow_bufs(ctx, ctx->cap_blockcnt, nbc, nbc, {dev_buf(ctx->d_blockcnt, nbc * 4), dev_buf(ctx->d_ublocktot, (nbc / SCAN_ITEMS + 2) * 4)}))) return rc;
  }
  size_t nout = nlw * nitems;
  if ((rc = grow_bufs(ctx, ctx->cap_partial, nout * 64, nout * 64, {dev_buf(ctx->d_partial, nout * 64 * sizeof(PointSum))}))) return rc;
  // h_out mapped + coherent, said explicitly: the export kernel writes it and the host polls the flag word without any runtime call in
  // between (with HIP_HOST_COHERENT=0 the default allocation is non-coherent and the poll would only end through its stream query)
  return grow_bufs(ctx, ctx->cap_out, nout, nout,
                   {dev_buf(ctx->d_out, (nout + 1) * sizeof(PointWords)),      // + one record: the input-validation flag word
                    host_buf(ctx->h_out, (nout + 1) * sizeof(PointWords), hipHostMallocMapped | hipHostMallocCoherent, &ctx->h_out_dev)});
}

// bytes of d_zblock the per-call memset clears: everything up to and including the heavy-bucket count, rounded up to 256 B
// (one fill kernel instead of an aligned body + a tail; the heavy ids it may touch are written later by k_chunk_desc)
static size_t zblock_clear_bytes(const Ctx* ctx) {
  size_t bytes = (size_t)((ctx->d_heavy + 1) - ctx->d_zblock) * 4;
  bytes = (bytes + 255) & ~(size_t)255;
  const size_t cap = ctx->cap_zblock * 4;
  return bytes < cap ? bytes : cap;
}

// profile 2: every phase is bracketed by hipEvents; 1 (default): only k_accumulate (the roofline kernel) -- each event record
// is a marker packet that costs the stream ~5.5 us, 8 of them were 4 % of a 2^16-term MSM; 0: none.
static int read_phase_events(Ctx* ctx, int profile) {
  for (int i = 0; i < CG1_NPHASE; ++i) ctx->phase_ms[i] = 0.f;
  if (profile >= 2) {
    for (int i = 0; i < CG1_NPHASE; ++i) HIPCHK(hipEventElapsedTime(&ctx->phase_ms[i], ctx->ev[i], ctx->ev[i + 1]));
  } else if (profile == 1) {
    HIPCHK(hipEventElapsedTime(&ctx->phase_ms[4], ctx->ev[4], ctx->ev[5]));
  }
  return CG1_OK;
}

static cg1h::fe fe_from_words12(const uint32_t w[12]) {     // already canonical and in the host's Montgomery form
  cg1h::fe r;
  for (int i = 0; i < 6; ++i) r.l[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
  return r;
}
static cg1h::jac jac_from_words(const PointWords& p) {
  if (p.inf) return cg1h::jac_identity();
  return cg1h::jac_from_xyzz(fe_from_words12(p.w[0]), fe_from_words12(p.w[1]), fe_from_words12(p.w[2]), fe_from_words12(p.w[3]));
}

}  // namespace cg1
