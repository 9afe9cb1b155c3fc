/* curdle_g1.h -- C ABI of libcurdle_g1.so: the MI355X-native BLS12-381 G1 / MSM engine that drops in
 * behind curdleproofs.pie's compute_MSM / MSMAccumulator and the G1Point surface of py_arkworks_bls12381.
 *
 * The reference has no FFI of its own: its boundary is the Python import
 *     from py_arkworks_bls12381 import G1Point, Scalar
 * (curdleproofs/curdleproofs/util.py:4, msm_accumulator.py:3, ...) plus
 *     from curdleproofs.msm_accumulator import MSMAccumulator, compute_MSM
 * (curdleproofs.py:17, ipa.py:23, grand_prod.py:17, same_msm.py:19, same_perm.py:14).
 * Each entry point below names the reference interface it stands behind.  The ctypes binding a
 * maintainer adds is shown in INTEGRATION.md (and lives in curdleproofs_pie_amd/_native.py).
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns an int status (CG1_OK == 0) unless it
 *     cannot fail; no exceptions cross the boundary; no global mutable state outside a cg1_ctx.
 *   - "point blob": 144 opaque bytes (host Jacobian X,Y,Z; 6x64-bit Montgomery limbs each).
 *   - "affine96": x || y, each a 48-byte little-endian integer < p in standard (non-Montgomery) form;
 *     the all-zero record encodes the identity ((0,0) is not on the curve).
 *   - "scalar32": 32-byte little-endian canonical Fr element (< r), as Scalar.to_le_bytes() returns.  The MSM entry
 *     points treat it as a plain integer and reject values >= 2^255 (CG1_ERR_ENCODING) instead of mis-summing them.
 *   - "compressed48": the 48-byte ZCash-format compression G1Point.to_compressed_bytes() returns.
 *   - device entry points fail with CG1_ERR_HIP when no GPU / HIP error; there is NO CPU fallback.
 */
#ifndef CURDLE_G1_H
#define CURDLE_G1_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CG1_OK            0
#define CG1_ERR_ARG       1   /* bad argument (size, window width, shard spec) */
#define CG1_ERR_HIP       2   /* HIP runtime error or no device; message via cg1_ctx_error */
#define CG1_ERR_ENCODING  3   /* malformed compressed48 / affine96 / scalar32 -> Python ValueError */
#define CG1_ERR_NOT_ON_CURVE 4
#define CG1_ERR_NOT_IN_SUBGROUP 5
#define CG1_ERR_COMM      6   /* multi-GPU exchange failed (rendezvous, socket, RCCL); message via cg1_comm_error */

#define CG1_POINT_BYTES 144
#define CG1_NPHASE 7          /* prepare, sort_count, sort_scatter, chunks, accumulate, seg_reduce, bit_tree(+D2H) */

typedef struct cg1_ctx cg1_ctx;

/* ---------------- host-side single-element G1 ops (G1Point operators; stub __init__.pyi:5-30) ---- */
void cg1_identity(uint8_t out[CG1_POINT_BYTES]);                      /* G1Point.identity()        util.py:11 */
void cg1_generator(uint8_t out[CG1_POINT_BYTES]);                     /* G1Point()                 util.py:9  */
void cg1_add(uint8_t out[CG1_POINT_BYTES], const uint8_t* a, const uint8_t* b);      /* __add__ */
void cg1_sub(uint8_t out[CG1_POINT_BYTES], const uint8_t* a, const uint8_t* b);      /* __sub__ */
void cg1_neg(uint8_t out[CG1_POINT_BYTES], const uint8_t* a);                        /* __neg__ */
void cg1_double(uint8_t out[CG1_POINT_BYTES], const uint8_t* a);
void cg1_mul(uint8_t out[CG1_POINT_BYTES], const uint8_t* a, const uint8_t scalar32[32]);  /* __mul__(Scalar) */
int  cg1_eq(const uint8_t* a, const uint8_t* b);                      /* __eq__; 1 equal, 0 not    util.py:17-18 */
int  cg1_is_identity(const uint8_t* a);
void cg1_compress(uint8_t out48[48], const uint8_t* a);               /* to_compressed_bytes       util.py:27-28 */
/* from_compressed_bytes (check_subgroup=1) / from_compressed_bytes_unchecked (0)   util.py:35-36,
 * msm_accumulator.py:65.  Returns CG1_OK or CG1_ERR_ENCODING / _NOT_ON_CURVE / _NOT_IN_SUBGROUP. */
int  cg1_decompress(uint8_t out[CG1_POINT_BYTES], const uint8_t in48[48], int check_subgroup);
void cg1_to_affine96(uint8_t out96[96], const uint8_t* a);
int  cg1_from_affine96(uint8_t out[CG1_POINT_BYTES], const uint8_t in96[96], int check_on_curve);
/* n affine96 records (as the batched device entry points return them; zeros = identity; not checked against the curve) -> n blobs */
int  cg1_batch_from_affine96(uint8_t* out_blobs, const uint8_t* in96, size_t n);
/* n point blobs -> n affine96 records with ONE field inversion (input marshalling for the MSM) */
void cg1_batch_to_affine96(uint8_t* out96, const uint8_t* blobs, size_t n);
/* n compressed48 -> n point blobs; stops at the first bad encoding and returns its status, *bad_index set */
int  cg1_batch_decompress(uint8_t* out_blobs, const uint8_t* in48, size_t n, int check_subgroup, size_t* bad_index);
void cg1_batch_compress(uint8_t* out48, const uint8_t* blobs, size_t n);

/* ---------------- device context --------------------------------------------------------------- */
int  cg1_device_count(void);                                         /* 0 when no GPU is visible */
cg1_ctx* cg1_ctx_create(int device);                                 /* NULL on failure (no GPU) */
/* the same with the context's compute / side streams confined to the CUs whose bit is set (bit i of word i / 32 = CU i) */
cg1_ctx* cg1_ctx_create_cu_mask(int device, const uint32_t* cu_mask, size_t n_words);
void cg1_ctx_destroy(cg1_ctx* ctx);
const char* cg1_ctx_error(const cg1_ctx* ctx);                       /* message of the last failure */
void* cg1_dev_malloc(cg1_ctx* ctx, size_t bytes);                    /* NULL on failure */
void cg1_dev_free(cg1_ctx* ctx, void* p);
int  cg1_h2d(cg1_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int  cg1_d2h(cg1_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* asynchronous H2D on the context's copy stream (src page-locked to overlap kernels); cg1_copy_fence orders everything
 * queued there so far before the next launch on the compute stream.  Neither blocks the host. */
int  cg1_h2d_async(cg1_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int  cg1_copy_fence(cg1_ctx* ctx);
int  cg1_stream_sync(cg1_ctx* ctx);                                  /* this context's compute stream only */
/* page-locked host memory for staging buffers (copies from it run at full PCIe rate); NULL on failure */
void* cg1_host_alloc(cg1_ctx* ctx, size_t bytes);
void cg1_host_free(cg1_ctx* ctx, void* p);
/* strided gather: `rows` records of `width` bytes lying `src_pitch` apart on the device -> `dst_pitch` apart on the host */
int  cg1_d2h_2d(cg1_ctx* ctx, void* dst_host, size_t dst_pitch, const void* src_dev, size_t src_pitch, size_t width, size_t rows);
int  cg1_ctx_sync(cg1_ctx* ctx);                                     /* hipDeviceSynchronize on the context's GPU */
int  cg1_ctx_device(const cg1_ctx* ctx);                             /* the HIP device ordinal the context was created on */
void* cg1_ctx_stream(cg1_ctx* ctx);                                  /* the context's compute stream (a hipStream_t), for callers ordering their own work */
/* Tuning and A/B switches of a context (defaults are the measured best; DESIGN.md section 9 has the measurements):
 *   MSM plan / phases   "chunk_len" "seg_m" "auto_plan" "stage_sort" "partition_sort" "big_bins" "wave_agg" "quad" "reduce_2d" "rowcol_quad"
 *                       "rowcol_quad_max" "fold_pass" "tree_half" "scan_one" "host_split" "horner_threads" "zero_copy" "batched_host_horner_max"
 *                       "batch_mul_quad_max" "batch_mul_host_max" "batch_mul_row" "horner_row" "small_row_tail" "sort_sub_bits" "rowcol_lgq" "tree_shift" "arm_helpers" "small_msm" (1: calls of <= 2048 terms run as ONE launch, k_msm_small; 0: the regime-A chain)
 *                       "lincomb_zero_copy" (1: GPU shares of cg1_lincomb_batch up to 4 096 terms are read by the kernel from mapped host memory, no staged copy),
 *                       "fold_quad" (1: quads fold a bucket's chunk sums at small bucket counts; 0: one lane per bucket, measured slower),
 *                       "tree_row" / "rowcol_row" (1: regime A's item sums, and for <= 2^18 buckets the cross-quad levels of the row / column sums, with one
 *                       limb per lane; 0: the quad kernels), "glv" / "glv_max_n" (the endomorphism split, see below: a PROMISE about the points, not a tuning
 *                       knob), "batched_split" / "batched_split_min_m" (regime B as two staggered half-batches: measured slower, default 0),
 *                       "split" (A/B switch, default 0: a call of >= 2^"split_min_log2n" terms as two launch chains -- high and low half of its windows -- on
 *                       two streams; measured slower than the single chain, profiles/r04_split_ab.txt)
 *   waiting             "blocking_sync" (sleep instead of spinning on the stream), "profile" (0: no events, 1: around k_accumulate, 2: every phase)
 *   codec               "decompress_waves" (2 | 3: waves per SIMD k_batch_decompress is compiled for)
 *   transcripts         "merlin_rows" (1: block program when the operation list fits), "merlin_sync" (1: lanes of a wave permute together),
 *                       "merlin_lanes" (1..64 transcripts per wave)
 *   verifier front-end  "fe_rows" (1: block program, 0: byte-level machine), "fe_timed" (shader-clock split of a launch), "fe_prio" (0..3)
 *   fixed-base tables   "fixed_slice" (terms per workgroup of k_table_msm, 1..128; 0: by the size of the call), "fixed_waves" (4, 8, 16 waves per
 *                       workgroup; 0: by the size of the call)
 *   Whisk shuffles      "whisk_resident_witness" (0 | 1, default 0: cg1_whisk_shuffle_prove_seeded keeps the permutation, k and every blinder it draws
 *                       on the device -- see there)
 *   test support        "alloc_fail_at" (k >= 1: the k-th allocation this context attempts from now on while growing a buffer it keeps between calls
 *                       -- its own, or a table's / front-end handle's -- fails as out of memory without reaching the runtime, then the parameter is
 *                       0 again; 0 disarms.  The refused call returns CG1_ERR_HIP and leaves the buffers it was growing empty, as a real failure does)
 * Unknown names and out-of-range values return CG1_ERR_ARG. */
int  cg1_ctx_set_param(cg1_ctx* ctx, const char* name, int value);

/* ---------------- the hot path: compute_MSM  (msm_accumulator.py:6-12) ------------------------- */
/* sum_i scalars[i] * points[i], inputs in host memory (copied to the device by the call). */
int cg1_msm(cg1_ctx* ctx, const uint8_t* points_affine96, const uint8_t* scalars32, size_t n,
            uint8_t out[CG1_POINT_BYTES]);
/* Same with inputs already resident in device memory (hipMalloc / cg1_dev_malloc / a torch tensor's
 * data_ptr).  window_c: 4..16 = uniform signed-digit windows of that width; -16..-4 = the balanced plan with cmax = -window_c
 * (ceil(256 / cmax) windows of width cmax or cmax - 1, so no window is thin); 0 = choose from n.
 * (shard_rank, shard_world): this call sums only windows w = shard_rank (mod shard_world) and returns
 * sum_w 2^(c w) S_w for those -- the per-GPU partial of a window-sharded MSM; (0,1) = the whole MSM.
 * window_c must then be the same on every rank. */
int cg1_msm_device(cg1_ctx* ctx, const void* d_points_affine96, const void* d_scalars32, size_t n,
                   int window_c, int shard_rank, int shard_world, uint8_t out[CG1_POINT_BYTES]);
/* Regime B -- a batch of n_msm INDEPENDENT small MSMs in one launch chain (e.g. the 5*ell+7-term final MSMs of
 * many MSMAccumulator.verify() calls, msm_accumulator.py:60-68; BASELINE config 3: 1024 x 627 terms).
 * MSM j sums terms [offsets[j], offsets[j+1]) of the concatenated inputs; offsets is a HOST array of
 * n_msm+1 entries with offsets[0] == 0; out_blobs receives n_msm point blobs.  window_c 4..9, 0 = auto. */
int cg1_msm_batched_device(cg1_ctx* ctx, const void* d_points_affine96, const void* d_scalars32,
                           const uint32_t* offsets, size_t n_msm, int window_c, uint8_t* out_blobs);
/* cg1_msm_device in two halves: _begin enqueues the context's launch chain and returns, _end waits, runs the host tail and
 * delivers the point (identity when n was 0).  Two contexts on one GPU keep two MSMs in flight: the next one's sort phases
 * run under this one's bucket accumulation, this one's reduction tail under the next one's. */
int cg1_msm_device_begin(cg1_ctx* ctx, const void* d_points_affine96, const void* d_scalars32, size_t n, int window_c,
                         int shard_rank, int shard_world);
int cg1_msm_device_end(cg1_ctx* ctx, uint8_t out[CG1_POINT_BYTES]);
int cg1_msm_batched(cg1_ctx* ctx, const uint8_t* points_affine96, const uint8_t* scalars32,
                    const uint32_t* offsets, size_t n_msm, uint8_t* out_blobs);
/* ---- the same call as the reference's callers make it: over the G1Point OBJECTS' own blobs (msm_accumulator.py:6-12 takes lists
 * of G1Point / Scalar; a G1Point here holds a 144-byte point blob, generally not normalised).  The blobs are uploaded as they are
 * and normalised on the device (k_prepare_blobs: Montgomery's trick, one inversion per GPU lane), so the host does no field
 * arithmetic per call.  all_normalised != 0: every blob has Z = 1 or Z = 0 (the caller checked): no inversion at all. */
int cg1_msm_blobs(cg1_ctx* ctx, const uint8_t* blobs144, const uint8_t* scalars32, size_t n, int all_normalised,
                  uint8_t out[CG1_POINT_BYTES]);
/* The same in two halves, for a caller that uploads slice by slice while it is still gathering the next one (cg1_h2d_async +
 * cg1_copy_fence): cg1_stage_reserve hands out the context's device staging for n blobs / n scalars (valid until the next call that
 * stages more), cg1_msm_blobs_device sums over blobs already resident there (or anywhere else on the device). */
int cg1_stage_reserve(cg1_ctx* ctx, size_t pts_bytes, size_t sc_bytes, void** d_pts, void** d_sc);
int cg1_msm_blobs_device(cg1_ctx* ctx, const void* d_blobs144, const void* d_scalars32, size_t n, int all_normalised,
                         uint8_t out[CG1_POINT_BYTES]);
/* A point vector resident on the device in the accumulation kernels' record format -- crs.vec_G / vec_H / vec_R ... are the
 * bases of dozens of compute_MSM calls of one prover (curdleproofs.py:77,94,95,319; grand_prod.py:54,90; ipa.py:97,98): made
 * once (upload + k_prepare_blobs), then each MSM uploads only its scalars.  cg1_msm_vec sums scalars[i] * vec[first + i], i < n. */
typedef struct cg1_vec cg1_vec;
cg1_vec* cg1_vec_create(cg1_ctx* ctx, const uint8_t* blobs144, size_t n, int all_normalised);   /* NULL on failure */
void   cg1_vec_destroy(cg1_vec* v);
size_t cg1_vec_len(const cg1_vec* v);
int cg1_msm_vec(cg1_ctx* ctx, const cg1_vec* vec, size_t first, size_t n, const uint8_t* scalars32, uint8_t out[CG1_POINT_BYTES]);
/* Host: n point blobs -> affine96 and / or compressed48 (either may be NULL) with ONE shared inversion: the map key
 * (msm_accumulator.py:54) and the affine form of MSMAccumulator.accumulate_check's bases from a single normalisation. */
int cg1_batch_normalize(const uint8_t* blobs, size_t n, uint8_t* out_affine96, uint8_t* out_comp48);

/* per-phase GPU times (hipEvents on the context's stream) and host Horner tail of the last MSM call */
int cg1_get_timings(const cg1_ctx* ctx, float phase_ms[CG1_NPHASE], float* host_tail_ms, int* window_c);

/* work counts of the last MSM call: non-zero signed digits sorted into buckets (= bucket additions + first-entry copies)
 * and the chunks k_accumulate ran (one copy each), so  mixed additions = entries - chunks */
int cg1_get_last_counts(const cg1_ctx* ctx, uint32_t* entries, uint32_t* chunks);
/* Which kernels of the reduction tail (everything behind k_accumulate) the last MSM call launched, as bit fields, low to high:
 * fold (2 bits: 0 none, 1 k_bucket_fold_quad, 2 k_bucket_fold) | row / column sums (3: 1 k_rowcol_quad_row, 2 k_rowcol_quad, 3 k_rowcol,
 * 4 k_seg_reduce) | k_rowcol_quad's lgq (3) | k_rowcol's use_quad (1) | k_seg_reduce's segment length (5) | tree (2: 1 k_small_tree_row,
 * 2 k_small_tree_quad, 3 k_small_tree) | waves of the tree's block (5) | export (2: 1 by k_small_tree_row, 2 k_export_host,
 * 3 hipMemcpyAsync) | Horner (3: 1 host, 2 k_msm_horner_row, 3 k_msm_horner_quad, 4 k_msm_horner) | host Horner threads (3; 0 = the worker
 * pool) | k_msm_small (2: 1 row_tail = 0, 2 row_tail = 1).  Written by plain host stores next to the launches; it exists for the tests,
 * which compare it with their own statement of the decision (tests/msm_tail_cases.py). */
uint32_t cg1_get_last_tail(const cg1_ctx* ctx);
/* k_accumulate launches of the last MSM call: 2 when it ran as two launch chains ("split"), 1, or 0 when k_msm_small served it */
int cg1_get_last_launches(const cg1_ctx* ctx);
/* The window plan of a width (window_c > 0: uniform; < 0: balanced with widths |c| and |c| - 1; glv: over the 128 positions of the halves of
 * the endomorphism split instead of 256): offset and width of every window, low to high.  Returns the number of windows (<= capacity) or -1.
 * No GPU involved: the CPU tests check that every plan tiles the bit positions from 0 without a gap. */
int cg1_plan_describe(int window_c, int glv, int* out_offsets, int* out_widths, int capacity);
/* What an MSM call would launch, from the engine's own planner (csrc/msm_plan.h).  No GPU and no context involved: the CPU tests compare it
 * with their models, the GPU tests with what the call then reports.
 * In:  switch_names / switch_values: n_switches cg1_ctx_set_param settings applied, in order, to a default switch set (MSM switches only);
 *      n, window_c, shard_rank, shard_world: as for cg1_msm_device; source_kind: 0 affine96, 1 point blobs, 2 a resident vector;
 *      n_msms: 0 = one MSM (cg1_msm_device and its kin), else a cg1_msm_batched_device call of n_msms MSMs over n terms in all, the largest
 *      of max_terms (window_c as for that call; the shard is ignored; neither half of the MSMs is taken to be empty);
 *      e_top: the highest exponent of an exported point that is not the identity (it sizes the host Horner's thread count).
 * Out (each may be NULL): *out_engine CG1_ENGINE_*; *out_c the plan's width as cg1_get_timings reports it (negative: balanced; 0: nothing
 *      runs); *out_glv whether the endomorphism split is on; *out_chunk_len the call's chunk length (0: no k_accumulate);
 *      *out_tail the word cg1_get_last_tail returns on the context after the call.  The two-chain forms describe the context's own chain:
 *      the upper windows, or the first n_msms / 2 MSMs taken as n / 2 terms.
 * Returns CG1_ERR_ARG where cg1_ctx_set_param would (unknown name, value out of range) or the call would (n, shard, width, batch size). */
#define CG1_ENGINE_NONE         0   /* nothing to launch: no terms */
#define CG1_ENGINE_SMALL        1   /* one k_msm_small launch */
#define CG1_ENGINE_CHAIN_A      2   /* the regime-A launch chain */
#define CG1_ENGINE_TWO_CHAINS_A 3   /* ... as two chains ("split") */
#define CG1_ENGINE_CHAIN_B      4   /* the regime-B launch chain */
#define CG1_ENGINE_TWO_CHAINS_B 5   /* ... as two chains ("batched_split") */
int cg1_msm_call_describe(const char* const* switch_names, const int* switch_values, int n_switches, size_t n, int window_c, int shard_rank,
                          int shard_world, int source_kind, size_t n_msms, size_t max_terms, int e_top,
                          int* out_engine, int* out_c, int* out_glv, uint32_t* out_chunk_len, uint32_t* out_tail);
/* hipEvent stopwatch on the context's compute stream: device time of everything enqueued between begin and end */
int cg1_timer_begin(cg1_ctx* ctx);
int cg1_timer_end(cg1_ctx* ctx, float* ms);

/* host-side wall times of the last MSM call: enqueue, wait-for-GPU, event readout, Horner tail (ms) */
int cg1_get_host_timings(const cg1_ctx* ctx, float host_ms[4]);

/* Segmented point sum -- the linear point sum of crs.py:64-65 (G_sum = reduce(a + b, vec_G, Z1), H_sum): out[j] = sum of the
 * points [offsets[j], offsets[j+1]); affine96 in and out; offsets is a HOST array of n_groups + 1 entries, offsets[0] == 0.
 * One wave per group. */
int cg1_batch_sum_device(cg1_ctx* ctx, const void* d_points_affine96, const uint32_t* offsets, size_t n_groups, void* d_out_affine96);
int cg1_batch_sum(cg1_ctx* ctx, const uint8_t* points_affine96, const uint32_t* offsets, size_t n_groups, uint8_t* out_affine96);
/* chip-wide v_mad_u64_u32 issue rate (lane-operations/s) with `waves_per_simd` resident waves: the peak roofline_int_mad is
 * priced against, measured in the same run as the benchmark (bench.py). */
int cg1_probe_mad_rate(cg1_ctx* ctx, int waves_per_simd, int iters, double* lane_ops_per_s);

/* ---------------- multi-GPU (SURVEY.md 8(b) "multi-GPU variants taking a device list", 8(e)) ---- */
/* The reference has no multi-device code; the contract is BASELINE.json's north_star: window buckets sharded over
 * the GPUs of one node, "final RCCL all-reduce of partial G1 sums".  RCCL has no elliptic-curve reduction, so the all-reduce is an
 * all-gather of ONE 144-byte point blob per rank + world-1 host additions on every rank (bit-identical on all ranks).
 *
 * (1) One process, several GPUs: ctxs[i] owns point shard i, resident on ITS device.  All launch chains are enqueued before
 *     any is waited for; out = the sum of the partials = compute_MSM (msm_accumulator.py:6-12) over the concatenation. */
int cg1_msm_multi_device(cg1_ctx* const* ctxs, size_t n_ctx, const void* const* d_points_affine96, const void* const* d_scalars32,
                         const size_t* n, int window_c, uint8_t out[CG1_POINT_BYTES]);
/* (2) One process per GPU (bench.py --gpus N, distributed.py).  A communicator is a TCP control channel on the loopback
 *     interface (rank 0 = hub: rendezvous, barriers, clocks, verdict gathers; alone it is the whole exchange when ranks rehearse on
 *     one GPU or on a CPU-only box) to which RCCL is attached for the data exchange on a GPU node.  No PyTorch anywhere.
 *       rank 0:  c = cg1_comm_create(0, world); publish cg1_comm_port(c) (file / env); cg1_comm_connect(c, NULL, 0, nonce, ms)
 *       others:  c = cg1_comm_create(r, world); cg1_comm_connect(c, "127.0.0.1", port, nonce, ms)   (CG1_ERR_COMM = wrong or
 *                not-yet-there listener: re-read the rendezvous and call again)
 *       all:     cg1_comm_attach_rccl(c, ctx)   -- ncclGetUniqueId on rank 0, id broadcast over the control channel,
 *                ncclCommInitRank on ctx's device; librccl.so is dlopen'ed here, on first use. */
typedef struct cg1_comm cg1_comm;
cg1_comm* cg1_comm_create(int rank, int world);                        /* NULL: bad arguments / cannot listen */
int  cg1_comm_port(const cg1_comm* c);                                 /* rank 0: the loopback port it listens on */
int  cg1_comm_rank(const cg1_comm* c);
int  cg1_comm_connect(cg1_comm* c, const char* host_ipv4, int port, uint64_t nonce, int timeout_ms);
int  cg1_comm_set_timeout(cg1_comm* c, int timeout_ms);                /* per collective; default 120 s */
int  cg1_comm_attach_rccl(cg1_comm* c, cg1_ctx* ctx);                  /* collective over all ranks */
const char* cg1_comm_transport(const cg1_comm* c);                     /* "rccl" once attached, else "socket" */
int  cg1_comm_world_seen(const cg1_comm* c);                           /* RCCL attached: ncclCommCount; else connected ranks */
const char* cg1_comm_error(const cg1_comm* c);
/* every rank contributes `bytes` host bytes, every rank receives world * bytes in rank order.  RCCL attached: one
 * ncclAllGather(uint8) on ctx's compute stream (payload staged through pinned memory); else the TCP star. */
int  cg1_comm_allgather(cg1_comm* c, const void* send, size_t bytes, void* recv);
int  cg1_comm_allgather_host(cg1_comm* c, const void* send, size_t bytes, void* recv);   /* always the control channel */
int  cg1_comm_barrier(cg1_comm* c);                                    /* control channel; pair with cg1_ctx_sync */
/* the "all-reduce of partial G1 sums": sum = partial_0 + ... + partial_{world-1}; all_blobs (may be NULL) gets the world blobs */
int  cg1_comm_allreduce_g1(cg1_comm* c, const uint8_t partial[CG1_POINT_BYTES], uint8_t sum[CG1_POINT_BYTES], uint8_t* all_blobs);
void cg1_comm_destroy(cg1_comm* c);

/* ---------------- batched scalar multiplication (`G1Point * Scalar`, vectorised) --------------- */
/* out[i] = scalars[i] * bases[i % nbase]; all device pointers; affine96 in and out.
 * nbase = 1 is the fixed-base case (get_random_point: G * random_scalar(), util.py:67-68). */
int cg1_batch_mul_device(cg1_ctx* ctx, const void* d_bases_affine96, size_t nbase, const void* d_scalars32,
                         void* d_out_affine96, size_t n);
/* General form: out[i] = addend[i] + scalars[i % nscalars] * bases[i % nbase]   (addend may be NULL).
 * nscalars = 1: same-scalar map  [R*k for R in vec_R]  (curdleproofs.py:310-311);
 * nscalars = 1 with addend = L:  fold  G_L[i] + G_R[i]*gamma  (ipa.py:142-146, same_msm.py:122-126);
 * per-index scalars:             G_i * beta^-i  (grand_prod.py:64-71). */
int cg1_batch_mul_add_device(cg1_ctx* ctx, const void* d_bases_affine96, size_t nbase, const void* d_scalars32,
                             size_t nscalars, const void* d_addend_affine96, void* d_out_affine96, size_t n);
/* same, all buffers in host memory (copied in and out by the call).  Which engine serves a call depends on the call alone ("batch_mul_host_max":
 * -1 = this rule, 0 = never the host, N = the host up to N outputs): up to 96 outputs the host's worker pool (cg1_batch_mul_add_pool: n scalar
 * multiplications of ~77 us over its threads, against a ~0.6 ms launch); up to 4 096 one WAVE per output with one limb per lane (k_batch_mul_row,
 * csrc/fp_row.h: ~0.55 ms whatever n is; "batch_mul_row" = 0 switches it off); beyond, one quad / one lane per output.  Every engine returns the
 * same records, byte for byte, and refuses the same inputs: a coordinate >= p is CG1_ERR_ENCODING; the curve equation is not checked. */
int cg1_batch_mul_add_pool(const uint8_t* bases_affine96, size_t nbase, const uint8_t* scalars32, size_t nscalars,
                           const uint8_t* addend_affine96, uint8_t* out_affine96, size_t n, int n_threads /* 0 = all */);
int cg1_batch_mul_add(cg1_ctx* ctx, const uint8_t* bases_affine96, size_t nbase, const uint8_t* scalars32, size_t nscalars,
                      const uint8_t* addend_affine96, uint8_t* out_affine96, size_t n);
/* Batched 48-byte decompression on the GPU: from_compressed_bytes_unchecked
 * (check_subgroup = 0, util.py:35-36, BufReader.read_g1 util.py:143-147) / from_compressed_bytes (= 1).
 * Device variant: per-point status byte (0 ok, CG1_ERR_ENCODING, _NOT_ON_CURVE, _NOT_IN_SUBGROUP), affine96 out.
 * Host variant: CG1_OK iff all n encodings are valid, else the first failing status and *bad_index. */
int cg1_batch_decompress_device(cg1_ctx* ctx, const void* d_in48, void* d_out_affine96, void* d_status, size_t n, int check_subgroup);
int cg1_batch_decompress_enqueue(cg1_ctx* ctx, const void* d_in48, void* d_out_affine96, void* d_status, size_t n, int check_subgroup);  /* no wait: pair with cg1_ctx_sync */
int cg1_batch_decompress_gpu(cg1_ctx* ctx, const uint8_t* in48, uint8_t* out_affine96, size_t n, int check_subgroup, size_t* bad_index);
/* Subgroup flags for k selected points of every proof of a decompressed batch (d_affine96: n_proofs x stride_points
 * records; offsets[j] < stride_points, k <= 16): d_flags[proof * k + j] = 1 iff that point is on the curve but outside G1.
 * The reference decodes unchecked (util.py:35-36) yet asserts the same-scalar equalities exactly (same_scalar.py:108);
 * weighting them randomly is sound only for points of G1, so flagged proofs get the exact check below.  Runs on the
 * context's side stream, ordered after what the compute stream holds so far; cg1_side_sync waits for it. */
int cg1_subgroup_flags_enqueue(cg1_ctx* ctx, const void* d_affine96, size_t stride_points, size_t n_proofs,
                               const uint32_t* offsets, size_t k, void* d_flags);
int cg1_side_sync(cg1_ctx* ctx);
/* Batched compression on the GPU: n affine96 records (as cg1_batch_mul_add_device / cg1_batch_decompress_device produce
 * them; zeros = identity) -> n compressed48 (to_compressed_bytes, util.py:27-28,120).  All device pointers. */
int cg1_batch_compress_device(cg1_ctx* ctx, const void* d_in_affine96, void* d_out48, size_t n);
/* deterministic synthetic scalars, uniform in [1, r-1] (util.py:21-24 distribution), from a 64-bit seed
 * (splitmix64 + rejection), device memory */
int cg1_gen_scalars_device(cg1_ctx* ctx, void* d_out_scalars32, size_t n, uint64_t seed);
/* roofline probe for the dominant kernel: `iters` dependent mixed adds per lane on `lanes` lanes;
 * returns elapsed ms in *ms */
int cg1_probe_madd(cg1_ctx* ctx, const void* d_points_affine96, size_t npts, size_t lanes, int iters, float* ms);

/* ---------------- deferred evaluation of the G1Point operators (north_star: "the prover/verifier keep their Python control flow
 * unchanged") -----------------------------------------------------------------------------------------------------------
 * The reference's loops call the operators one at a time: 585 x from_compressed_bytes_unchecked per verification
 * (whisk_interface.py:96-106 -> util.py:35-36), G_L[i] + G_R[i] * gamma (ipa.py:142-146, same_msm.py:122-126), R * k
 * (curdleproofs.py:310-311), G_i * beta^-i (grand_prod.py:64-71).  The Python face (py_arkworks_bls12381.py) answers them with
 * deferred values and evaluates whole batches through the entry points below when bytes or a comparison are asked for.
 *
 * cg1_validate_compressed: what from_compressed_bytes_unchecked must decide AT THE CALL (util.py:35-36 raises there;
 * test_curdleproofs.py:170-176,211-213): compression flag, x < p, and x^3 + 4 a square -- by its Jacobi symbol, no square root.
 * CG1_OK (is_identity: the infinity flag was set), CG1_ERR_ENCODING, CG1_ERR_NOT_ON_CURVE. */
int cg1_validate_compressed(const uint8_t in48[48], int* is_identity);
int cg1_fp_jacobi(const uint8_t le48[48]);               /* Jacobi symbol (a / p) of a 48-byte little-endian a < p: 1, -1, 0; 2 = a >= p */
/* n encodings (already validated, or not: the first failing index / status come back) -> blobs and / or affine96, on the worker pool */
int cg1_batch_decompress_pool(const uint8_t* in48, size_t n, uint8_t* out_blobs144, uint8_t* out_affine96, int n_threads, size_t* bad_index);
/* the same on the GPU for up to 8 192 encodings (k_batch_decompress_row: one DPP row per point, the square-root chain with one limb per
 * lane; ~0.15 ms whatever n is, through the context's mapped scratch): what the deferred layer uses for batches of >= 192 encodings */
int cg1_batch_decompress_rows(cg1_ctx* ctx, const uint8_t* in48, size_t n, uint8_t* out_blobs144, uint8_t* out_affine96, size_t* bad_index);
/* out_flags[i] = 1 iff affine96 point i (on the curve; zeros = identity) lies in the prime-order subgroup G1: [z^2]P == phi(P) + P.
 * Only for such bases may the coefficient of a deferred product be reduced mod r (`(P * a) * b` == P * (a b mod r)). */
int cg1_batch_subgroup_pool(const uint8_t* affine96, size_t n, uint8_t* out_flags, int n_threads);
/* the same flags; 32 .. 4 096 points and a GPU context: one wave per point with one limb per lane (k_subgroup_row: ~0.25 ms whatever n is);
 * otherwise the pool.  *on_device (may be NULL): 1 when the GPU served the call.  Coordinates >= p: CG1_ERR_ENCODING on both paths. */
int cg1_batch_subgroup(cg1_ctx* ctx, const uint8_t* affine96, size_t n, uint8_t* out_flags, int* on_device);
/* out_j = sum_{t in [offsets[j], offsets[j+1])} scalars32[t] * (+/-) bases[term_base[t] & 0x7fffffff]  (bit 31 of term_base: the negated
 * base); offsets: n_out + 1 host entries, offsets[0] == 0.  path 0 = choose from the batch (never from the machine), 1 = the host's worker
 * pool, 2 = the GPU (cg1_msm_batched_device over the gathered terms).  ctx may be NULL for paths 0 / 1 (then always the pool).  Outputs
 * (each may be NULL) are normalised: point blobs with Z = 1, affine96, compressed48.  *path_used: 1 pool, 2 GPU, 3 = both at once
 * (combinations of >= 4 weighted terms in one k_msm_small launch, the smaller ones on the pool while it runs). */
int cg1_lincomb_batch(cg1_ctx* ctx, const uint8_t* bases_affine96, size_t n_bases, const uint32_t* offsets, size_t n_out,
                      const uint32_t* term_base, const uint8_t* term_scalars32, int path, uint8_t* out_blobs144, uint8_t* out_affine96,
                      uint8_t* out_comp48, int* path_used);
int cg1_lincomb_batch_pool(const uint8_t* bases_affine96, size_t n_bases, const uint32_t* offsets, size_t n_out, const uint32_t* term_base,
                           const uint8_t* term_scalars32, uint8_t* out_blobs144, uint8_t* out_affine96, uint8_t* out_comp48, int n_threads);

/* ---------------- the endomorphism split (csrc/glv.h) -----------------------------------------------------------------------
 * For P in the prime-order subgroup phi(x, y) = (beta x, y) equals lambda P, lambda = z^2 - 1.  With the context parameter "glv" != 0 the
 * CALLER VOUCHES that every point of its MSM calls lies in G1 (CRS points, outputs of earlier MSMs, points that passed the subgroup
 * test); the engine may then run an MSM over the 2n entries (k1, P_i), (k2, phi(P_i)) of the 127-bit halves k = k1 + k2 lambda: the same
 * bucket additions, half the windows (half the doublings of the Horner tail).  1 = where it pays: the single-launch kernel (n <= 1 024,
 * also the <= 64 MSMs of one cg1_msm_batched* / cg1_lincomb_batch launch), the regime-B chain, and regime A up to "glv_max_n" terms (2^14: above, the second
 * half of the table costs more than the tail gains, profiles/r05_glv_ab.txt); 2 = wherever it can (A/B runs).  Outside G1
 * phi(P) != lambda P and the result would be wrong: the default is 0, and the Python face switches it on for single calls whose bases it
 * has certified.
 * cg1_glv_split: the split of one scalar (< 2^255, little-endian) as the digit kernels compute it -- magnitudes < 2^127 and signs --
 * for tests: (-1)^neg1 k1 + (-1)^neg2 k2 lambda == k (mod r). */
void cg1_glv_split(const uint8_t scalar32[32], uint8_t k1_16[16], uint8_t k2_16[16], int* neg1, int* neg2);

/* The lone-wave addition probe (csrc/fp_row.h): `waves` waves each run `iters` DEPENDENT EC additions; mode 0 = one lane per addition (the
 * formulas k_accumulate uses), 1 = one DPP quad per addition (g1_quad.h: the latency-bound kernels), 2 = one limb per lane, the four
 * products of a stage on the four rows of the wave.  *ms = device time of one launch (best of reps); out_blob144 = wave 0's result. */
int cg1_probe_add_chain(cg1_ctx* ctx, int mode, const uint8_t* two_points_affine96, size_t waves, int iters, int reps,
                        uint8_t* out_blob144, float* ms);

/* The arithmetic probes: the device's base-field, group and scalar-field operations over operands taken AS GIVEN -- raw limbs / raw
 * Montgomery words in, raw results out, nothing normalised or exported on the way -- so that a test can feed each of them the carry
 * patterns, lazy forms and multiples of p its callers can reach (tests/test_field_edges_gpu.py).  Host buffers, n <= 4 096 per call; the
 * caller guarantees the operation's preconditions.
 * cg1_probe_fp_ops: in_limbs = n tuples of four 14-limb vectors a, b, c, d; out_limbs = n 14-limb results; out_flags = n words.  form 0 =
 * one lane per tuple (csrc/fp28.h), 1 = one limb per lane, one DPP row per tuple (csrc/fp_row.h).  to_words / to_host_words: form 0 only,
 * 12 words out (then two zero words).  is_zero_mod_p takes kmax = 6, 8, 10 or 14 on one lane and 6 on rows, the values the product code passes
 * (CG1_ERR_ARG otherwise); the other operations ignore kmax.
 * cg1_probe_g1_ops: in_xyzz = n pairs of XYZZ records of CG1_PROBE_XYZZ_WORDS words (X, Y, ZZ, ZZZ as 14 limbs each, then inf, then
 * padding), out_xyzz = n records.  op 0 = a + b, 1 = 2 a.  form 0 = one lane (csrc/g1_xyzz.h), 1 = a DPP quad (csrc/g1_quad.h), 2 = a wave
 * with one limb per lane (csrc/fp_row.h; limbs come back nearly normal, <= 2^28 + 3).
 * cg1_probe_fr_ops / cg1_fr_ops_host: csrc/fr.h as compiled for the device / for the host, one operation over n items of 64 bytes, 64
 * bytes out each: the result in bytes 0..31, from_le32's boolean as a 64-bit word at byte 32.  mul, add, sub, neg, inv, inv_binary take
 * and return raw Montgomery words (operands at bytes 0 and 32; mul accepts any 256-bit first operand); from_le32 / to_le32 read bytes
 * 0..31, from_le64_wide all 64; pow_u64 has its exponent at byte 32. */
#define CG1_FP_OP_MUL 0
#define CG1_FP_OP_SQR 1
#define CG1_FP_OP_MUL2 2
#define CG1_FP_OP_NORM 3
#define CG1_FP_OP_IS_ZERO 4
#define CG1_FP_OP_INV 5
#define CG1_FP_OP_TO_WORDS 6
#define CG1_FP_OP_TO_HOST_WORDS 7
#define CG1_PROBE_XYZZ_WORDS 64
#define CG1_FR_OP_MUL 0
#define CG1_FR_OP_ADD 1
#define CG1_FR_OP_SUB 2
#define CG1_FR_OP_NEG 3
#define CG1_FR_OP_FROM_LE32 4
#define CG1_FR_OP_FROM_LE64_WIDE 5
#define CG1_FR_OP_TO_LE32 6
#define CG1_FR_OP_INV 7
#define CG1_FR_OP_INV_BINARY 8
#define CG1_FR_OP_POW_U64 9
#define CG1_FR_OP_COUNT 10
int cg1_probe_fp_ops(cg1_ctx* ctx, int form, int op, uint32_t kmax, const uint32_t* in_limbs, size_t n, uint32_t* out_limbs, uint32_t* out_flags);
int cg1_probe_g1_ops(cg1_ctx* ctx, int form, int op, const uint32_t* in_xyzz, size_t n, uint32_t* out_xyzz);
int cg1_probe_fr_ops(cg1_ctx* ctx, int op, const uint8_t* in, size_t n, uint8_t* out);
int cg1_fr_ops_host(int op, const uint8_t* in, size_t n, uint8_t* out);

/* ---------------- native Merlin transcript (host C++) ------------------------
 * Stands behind merlin_transcripts/merlin_transcripts/{merlin_transcript.py:6-24, strobe.py:16-107,
 * keccak.py:16-66} and curdleproofs/curdleproofs/curdleproofs_transcript.py:7-28.
 * `state` is a caller-owned CG1_MERLIN_STATE_BYTES blob; copying the blob forks the transcript. */
#define CG1_MERLIN_STATE_BYTES 208
void cg1_keccak_f1600(uint8_t* state200);              /* keccak.py:16-66, one permutation */
void cg1_keccak_f1600_x8(uint64_t* lanes);               /* eight states at once, lane w of state k at lanes[8*w + k] (AVX-512 when present) */
void cg1_keccak_f1600_x8_states(uint8_t* const* states200, int live);   /* 1..8 sponges permuted where they lie */
void cg1_strobe_new(uint8_t* state, const uint8_t* protocol_label, size_t len);                 /* Strobe128.new */
int  cg1_strobe_meta_ad(uint8_t* state, const uint8_t* data, size_t len, int more);
int  cg1_strobe_ad(uint8_t* state, const uint8_t* data, size_t len, int more);
int  cg1_strobe_prf(uint8_t* state, uint8_t* out, size_t len, int more);
int  cg1_strobe_key(uint8_t* state, const uint8_t* data, size_t len, int more);
void cg1_merlin_init(uint8_t* state, const uint8_t* label, size_t len);                          /* MerlinTranscript(label) */
void cg1_merlin_append(uint8_t* state, const uint8_t* label, size_t label_len, const uint8_t* msg, size_t msg_len);
void cg1_merlin_append_list(uint8_t* state, const uint8_t* label, size_t label_len, const uint8_t* items,
                            size_t item_len, size_t count);                                       /* append_list */
void cg1_merlin_challenge(uint8_t* state, const uint8_t* label, size_t label_len, uint8_t* out, size_t out_len);
/* get_and_append_challenge: 32 LE bytes of a canonical non-zero Fr element, already re-appended */
void cg1_merlin_challenge_scalar(uint8_t* state, const uint8_t* label, size_t label_len, uint8_t out32[32]);

/* ---------------- batch verifier front-end of the shuffle argument (host C++) ----------
 * Stands behind CurdleProofsProof.verify (curdleproofs/curdleproofs/curdleproofs.py:160-246) and its
 * sub-verifiers same_perm.py:75-121, grand_prod.py:161-218, ipa.py:156-236, same_scalar.py:71-111,
 * same_msm.py:146-227, on the wire format of WhiskShuffleProof.from_bytes (whisk_interface.py:64-69) and of the
 * trackers (whisk_interface.py:96-100).  It does NOT verify by itself: it reduces each proof to the statement
 *        sum_k own_scalars[k] * own_points[k]  +  sum_j crs_scalars[j] * crs_points[j]  ==  identity
 * which the caller checks with cg1_batch_decompress_device + cg1_msm_device (many proofs merged: add the CRS
 * scalar vectors) or cg1_msm_batched_device (independently).  Python driver: curdleproofs_pie_amd/shuffle_verifier.py.
 *
 * Layouts (ell trackers, n = ell + 4 = 2^lg):
 *   crs bytes       (ell+9) x 48: vec_G | vec_H(4) | H | G_t | G_u | G_sum | H_sum  = CurdleproofsCrs.to_bytes (crs.py:92-101)
 *   instance        4*ell x 48:   vec_R | vec_S | vec_T | vec_U (tracker r_G / k_r_G encodings, pre then post)
 *   proof           cg1_shuffle_proof_bytes(): M | A | cm_T | cm_U | R | S | same_perm | same_scalar | same_msm
 *   own points      cg1_shuffle_points_per_proof() = 4*ell + 19 + 10*lg encodings: the instance, then the proof's
 *                   points in wire order; own scalars use the same indexing, crs scalars the crs-bytes indexing
 *   weights         12 x scalar32 per proof: the random rho of each of the 8 accumulated checks
 *                   (msm_accumulator.py:43) and of the 4 same-scalar equalities (same_scalar.py:108)
 *   status          0 = prepared; CG1_SHUFFLE_* = rejected before any group arithmetic (its scalars are zeroed)
 *   challenges      optional (may be NULL), for parity tests: alpha_p beta_p alpha_g beta_g alpha_ipa beta_ipa
 *                   alpha_samescalar alpha_samemsm | gamma_ipa[lg] | gamma_samemsm[lg] | vec_a[ell]
 */
#define CG1_SHUFFLE_BAD_SCALAR   1   /* an Fr field of the proof is >= r   (Scalar.from_le_bytes raises, util.py:149-153) */
#define CG1_SHUFFLE_BAD_POINT    2   /* A, cm_T.T_1, cm_U.T_1 or B does not decode (util.py:143-147)                     */
#define CG1_SHUFFLE_T0_INFINITY  3   /* vec_T[0] is the identity (curdleproofs.py:173-174)                               */
#define CG1_SHUFFLE_BAD_WEIGHT   4   /* a caller-supplied weight is >= r                                                  */
typedef struct cg1_shuffle_crs cg1_shuffle_crs;
cg1_shuffle_crs* cg1_shuffle_crs_create(const uint8_t* crs_bytes, size_t ell, size_t n_blinders);   /* NULL: bad sizes / encoding */
void   cg1_shuffle_crs_destroy(cg1_shuffle_crs* crs);
size_t cg1_shuffle_proof_bytes(const cg1_shuffle_crs* crs);
size_t cg1_shuffle_points_per_proof(const cg1_shuffle_crs* crs);
size_t cg1_shuffle_crs_points(const cg1_shuffle_crs* crs);
size_t cg1_shuffle_challenges_per_proof(const cg1_shuffle_crs* crs);
/* decoded96 (may be NULL): per proof, at decoded96 + i*decoded_stride, the 8 consecutive own points 4*ell+1 .. 4*ell+8
 * (A T_1 T_2 U_1 U_2 R S B) in affine96 form as cg1_batch_decompress_device produced them (one strided D2H copy).
 * Of these the verifier needs A, T_1, U_1, B as group elements (A' = A + T_1 + U_1, curdleproofs.py:204; D,
 * grand_prod.py:186).  NULL: the host decodes those four itself (4 square roots per proof). */
int cg1_shuffle_prepare(const cg1_shuffle_crs* crs, size_t n_proofs, const uint8_t* instances, const uint8_t* proofs,
                        const uint8_t* weights, const uint8_t* decoded96, size_t decoded_stride,
                        uint8_t* out_points48, uint8_t* out_scalars32, uint8_t* out_crs_scalars32,
                        int32_t* status, uint8_t* out_challenges32, int n_threads /* 0 = all cores */);
/* 1 (default): cg1_shuffle_prepare advances 16 proofs' transcripts in step, their Keccak-f permutations eight at a time
 * (AVX-512 when present); 0: one transcript at a time.  Same output bytes either way. */
void cg1_shuffle_set_grouped(int on);
/* threads used when n_threads = 0: usable CPUs (affinity mask capped by the cgroup CPU quota; env CURDLE_G1_THREADS overrides) */
size_t cg1_shuffle_default_threads(void);
/* Batched Merlin transcripts on the device (HIP half): n transcripts, one per GPU lane, all starting from
 * init_state208 (what cg1_merlin_init left on the host) and all running the same operation list on their own data rows:
 *   kind 0  append_message(label, data_row[data_off .. data_off + len))                      merlin_transcript.py:11-15
 *   kind 1  challenge_bytes(label, len) -> out_row[out_off ..]                                merlin_transcript.py:20-24
 *   kind 2  get_and_append_challenge(label) -> 32 bytes at out_row[out_off ..]                curdleproofs_transcript.py:15-25
 *   kind 3  append_message(label, out_row[out_off .. out_off + len))   (a value the transcript produced itself)
 * d_states_out (optional): the n final 208-byte state blobs, interchangeable with the host functions above. */
typedef struct cg1_merlin_op {
  uint8_t kind, label_len;
  uint16_t pad;
  uint32_t len, data_off, out_off;
  uint8_t label[32];
} cg1_merlin_op;
/* Keccak passes the slowest wave of the last cg1_merlin_batch_device call executed (the lanes of a wave permute together;
 * a shuffle-shaped program needs ~750 permutations per transcript). */
int cg1_merlin_last_passes(const cg1_ctx* ctx);
/* Which kernel served that call: 2 = block program (whole rate blocks per pass; the default when the operation list fits its row format:
 * challenges of at most 164 bytes, 4-byte aligned output offsets, at most four self-produced pieces per block), 1 = byte-level state
 * machine ("merlin_rows" = 0, or the program does not fit), 0 = one lane at a time ("merlin_sync" = 0, or more than 48 distinct labels). */
int cg1_merlin_last_kernel(const cg1_ctx* ctx);
/* Host only, test support: ONE transcript of that interface run through the block program on the CPU (the tables the device kernels
 * consume, walked the way they walk them); CG1_ERR_ARG when the operation list does not fit the row format. */
int cg1_merlin_block_program_emulate(const uint8_t* init_state208, const cg1_merlin_op* ops, size_t nops, const uint8_t* data_row, size_t data_bytes,
                                     uint8_t* out_row, size_t out_bytes, uint8_t* state_out208 /* may be NULL */, uint32_t* passes);
/* Host only, test support: n (1..16) transcripts, all MerlinTranscript(label), run IN STEP through the grouped host path of
 * cg1_shuffle_prepare (csrc/merlin_group.h: one operation at a time over all of them, Keccak-f eight at a time).  Takes what that path
 * takes and nothing else: kind 0 with len <= 64, kind 2, labels without a zero byte; anything else is CG1_ERR_ARG.  Transcript k
 * reads data + k * data_stride and writes its 32-byte challenges to out + k * out_stride (at each op's out_off) and, when states is
 * given, its final blob to states + k * 208 (byte 202, the current operation's flags, which the group does not keep: what either
 * operation leaves there). */
int cg1_merlin_group_run(const uint8_t* label, size_t label_len, const cg1_merlin_op* ops, size_t nops, const uint8_t* data,
                         size_t data_stride, uint8_t* out, size_t out_stride, uint8_t* states /* may be NULL */, size_t n);
int cg1_merlin_batch_device(cg1_ctx* ctx, const uint8_t* init_state208, const cg1_merlin_op* ops, size_t nops, const void* d_data,
                            size_t data_stride, void* d_out, size_t out_stride, void* d_states_out, size_t n);

/* Scalar rows on the device (ipa.py:155-186,216,227-229; same_msm.py:146-182,213; grand_prod.py:64-71;
 * msm_accumulator.py:43-58).  cg1_shuffle_prepare_inputs is cg1_shuffle_prepare without the row expansion: per proof it emits
 * cg1_shuffle_rowin_scalars(crs) 32-byte scalars (the transcript's challenges, their inverses, beta^-1, inner_prod, the
 * proof's Fr fields, the weights).  cg1_shuffle_rows_device expands them on the GPU into the same rows, byte for byte:
 * d_out_scalars receives n_proofs x points_per_proof own-point scalars followed by the crs_points sums over the live proofs;
 * d_crs_rows the per-proof CRS rows; d_status_out the final per-proof codes (host code, or CG1_SHUFFLE_BAD_POINT when
 * d_point_status -- the decompression verdicts of the proof's own points -- has a non-zero byte). */
size_t cg1_shuffle_rowin_scalars(const cg1_shuffle_crs* crs);
int cg1_shuffle_prepare_inputs(const cg1_shuffle_crs* crs, size_t n_proofs, const uint8_t* instances, const uint8_t* proofs,
                               const uint8_t* weights, const uint8_t* decoded_affine96, size_t decoded_stride, uint8_t* out_points48,
                               uint8_t* out_rowin32, int32_t* status, int n_threads);
int cg1_shuffle_rows_device(cg1_ctx* ctx, size_t ell, size_t lg, size_t n_proofs, const void* d_rowin, const void* d_host_status,
                            const void* d_point_status, void* d_out_scalars, void* d_crs_rows, void* d_status_out);
/* Exact (unweighted) evaluation on the host of the equalities the reference asserts directly, for proofs that carry a
 * point outside G1 (cg1_subgroup_flags_enqueue / CG1_ERR_NOT_IN_SUBGROUP): the four same-scalar equalities of one shuffle
 * proof (same_scalar.py:101-108; *ok = 1 iff all hold), and the two equalities of one tracker-opening proof
 * (opening.py:73-76).  Points are decoded unchecked, scalars act as integers in [0, r), as in the reference. */
/* The front-end ON THE DEVICE (csrc/kernels_frontend.h): what cg1_shuffle_prepare_inputs does on the host -- the Fiat-Shamir transcript
 * (curdleproofs_transcript.py:15-25 over merlin_transcripts), the grand-product scalar (same_perm.py:98-101), D (grand_prod.py:157) and
 * A' (curdleproofs.py:210) with their encodings, inner_prod (grand_prod.py:164-166), the challenge inverses -- one proof per lane on the
 * wire points already in HBM.  Same outputs, byte for byte: the row-input blocks and the per-proof front-end codes.
 * cg1_shuffle_gather_aux collects what the kernel needs besides the points: per proof r_p c_final d_final z_k z_t z_u x_final | 12 weights. */
typedef struct cg1_shuffle_fe cg1_shuffle_fe;
cg1_shuffle_fe* cg1_shuffle_fe_create(cg1_ctx* ctx, size_t ell, size_t lg, const uint8_t* crs_affine96, const uint8_t* crs48);   /* NULL on failure */
void   cg1_shuffle_fe_destroy(cg1_shuffle_fe* fe);
size_t cg1_shuffle_fe_aux_bytes(void);
/* The kernel runs a BLOCK PROGRAM: the transcript of a given ell cut on the host into the rate blocks between two permutations
 * ("nodes"; 0 = this ell does not fit the format and the byte-level state machine is used; cg1_ctx_set_param("fe_rows", 0) forces
 * that one).  _last_passes: Keccak passes of the slowest wave of the last launch enqueued on ctx (waits for the stream). */
size_t cg1_shuffle_fe_nodes(const cg1_shuffle_fe* fe);
int    cg1_shuffle_fe_emulate_to_first_barrier(size_t ell, size_t lg, const uint8_t* crs_h48, const uint8_t* wire, uint8_t* out_row, size_t out_row_bytes,
                                               uint32_t* passes);   /* host only, test support: the block program of ONE proof walked on the CPU up to the grand-product step; out_row >= (cg1_shuffle_rowin_scalars + 6) * 32 bytes, the drawn challenges in their slots */
int    cg1_shuffle_fe_program_shape(size_t ell, size_t lg, uint32_t* out4);   /* host only: {operations, nodes (0 = does not fit), squeeze nodes, max late pieces per node} */
size_t cg1_shuffle_fe_last_passes(cg1_shuffle_fe* fe, cg1_ctx* ctx);
void   cg1_shuffle_fe_last_split(const cg1_shuffle_fe* fe, uint32_t* out7);   /* ("fe_timed" launches) that wave's shader clocks / 256: late pieces + row loads issued | Keccak-f | whole passes | draw + range check | X_GPROD | X_DA | X_FINAL */
int cg1_shuffle_gather_aux(const cg1_shuffle_crs* crs, size_t n_proofs, const uint8_t* proofs, const uint8_t* weights, uint8_t* out_aux);
int cg1_shuffle_fe_enqueue(cg1_shuffle_fe* fe, cg1_ctx* ctx, size_t n, const void* d_wire48, const void* d_pts_affine96, const void* d_aux,
                           void* d_rowin, void* d_status, int lanes_per_wave /* 1..64 transcripts per wave; 0 = 64 */);
int cg1_shuffle_exact_same_scalar(const cg1_shuffle_crs* crs, const uint8_t* instance, const uint8_t* proof, int* ok);
int cg1_opening_exact(const uint8_t* tracker96 /* r_G | k_r_G */, const uint8_t* k_commitment48, const uint8_t* proof128, int* ok);
/* the same check with the batch path's status code: 0 accepted, CG1_SHUFFLE_BAD_SCALAR, CG1_SHUFFLE_BAD_POINT, 6 = an equality fails.  What
 * OpeningBatchVerifier uses for a handful of proofs -- IsValidWhiskOpeningProof itself (whisk_interface.py:147-169) is a batch of ONE: five
 * single decompressions and four scalar multiplications on the host (~0.4 ms) against ~2.4 ms of dependent GPU launches. */
int cg1_opening_exact_status(const uint8_t* tracker96, const uint8_t* k_commitment48, const uint8_t* proof128, int* status);
/* Exact relations in bulk: ok[i] = 1 iff sum_j (+-) k_j * P_j over the (at most CG1_EXACT_TERMS) terms of relation i is the identity --
 * what the two entries above evaluate for one proof, for any number of relations over flat arrays:
 *   points96     n_points affine96 records (x | y, 48-byte little-endian standard form; all-zero = the identity); ANY point of the curve,
 *                inside G1 or not -- nothing is folded, split or reduced, a scalar is its 256-bit integer
 *   scalars32    n_scalars 32-byte little-endian scalars (n_scalars < CG1_EXACT_ONE)
 *   terms        n_relations x CG1_EXACT_TERMS records of two uint32: { point index, or CG1_EXACT_NONE for "no term" ; scalar index, or
 *                CG1_EXACT_ONE for the scalar one (no ladder is paid for it), with CG1_EXACT_NEG set for a minus sign }.  HOST memory in
 *                both entries: every index is checked before anything runs (cg1_exact_relations_check; CG1_ERR_ARG, nothing written).
 * cg1_exact_relations_device: d_points96, d_scalars32 and d_ok are DEVICE memory.  The records are host memory here too -- not a device
 * array -- BECAUSE every index is checked on the host before the launch; they travel through one of two page-locked blocks the context
 * keeps and uses in turn, then ONE launch (k_exact_relations: a wave per relation, the terms of a relation share one ladder's
 * doublings) on the context's stream.  It allocates nothing once the kept blocks have grown and waits for no kernel and not for its own
 * upload: the caller synchronises the stream before reading d_ok (a staging block is reused only after the upload it carried two calls
 * earlier has left it -- the only wait inside, and none when fewer than three calls are in flight).  The device entry ASSUMES what
 * cg1_batch_decompress_device produces: canonical coordinates (< p) of points on the curve; it cannot refuse a coordinate >= p as the
 * host twin does (the kernel would compute with the unreduced value), and neither entry tests the curve equation.
 * cg1_exact_relations: the host twin over host arrays on the worker pool (n_threads <= 0: all of it); a coordinate >= p: CG1_ERR_ENCODING.
 * cg1_exact_gather_device: dst block j (at j * dst_stride_bytes) = src block idx[j] (at idx[j] * src_stride_bytes; a stride of 0 repeats one
 * block), block_bytes each, with the bytes [clear_off, clear_off + clear_bytes) of every copied block zeroed -- the flagged subset of a batch
 * compacted on the device (row-input blocks with the same-scalar weights cleared, own points, CRS points repeated) for the weighted pass over
 * it.  Device memory in and out, idx in host memory and checked against n_src_blocks there (CG1_ERR_ARG; also for sizes that are no
 * multiple of 4 or a block longer than a stride); one launch on the context's stream through the same staging, no wait for it.
 * cg1_opening_challenges: the transcript half of cg1_opening_exact_status for n proofs on the worker pool: out_c32[i] = the challenge c of
 * proof i (trackers96 n x (r_G | k_r_G), k_commitments48, proofs128 as cg1_opening_exact takes them; the encodings are absorbed as they
 * are, decodable or not). */
#define CG1_EXACT_TERMS 4
#define CG1_EXACT_NEG   0x80000000u
#define CG1_EXACT_ONE   0x7fffffffu
#define CG1_EXACT_NONE  0xffffffffu
int cg1_exact_relations_check(const uint32_t* terms, size_t n_relations, size_t n_points, size_t n_scalars);
int cg1_exact_relations(const uint8_t* points96, size_t n_points, const uint8_t* scalars32, size_t n_scalars, const uint32_t* terms,
                        size_t n_relations, uint8_t* ok, int n_threads);
int cg1_exact_relations_device(cg1_ctx* ctx, const void* d_points96, size_t n_points, const void* d_scalars32, size_t n_scalars,
                               const uint32_t* terms, size_t n_relations, void* d_ok);
int cg1_exact_gather_device(cg1_ctx* ctx, const void* d_src, size_t n_src_blocks, size_t src_stride_bytes, const uint32_t* idx, size_t n_idx,
                            void* d_dst, size_t dst_stride_bytes, size_t block_bytes, size_t clear_off, size_t clear_bytes);
int cg1_opening_challenges(const uint8_t* trackers96, const uint8_t* k_commitments48, const uint8_t* proofs128, size_t n, uint8_t* out_c32,
                           int n_threads);
/* just the gather step: every proof's own points (instance, then the proof's points in wire order) */
int cg1_shuffle_gather_points(const cg1_shuffle_crs* crs, size_t n_proofs, const uint8_t* instances, const uint8_t* proofs,
                              uint8_t* out_points48);
/* A chain of shuffles over one tracker set that stays on the device in decoded form (shuffle_chain.py).  Block j of a batch reads
 * pre_j = [set[i] for i in indices_j] before any of its own writes, then writes set[indices_j[t]] = post_j[t], t = 0 .. ell - 1 in order
 * (indices of a block may repeat: reads first, the last write wins).
 * cg1_chain_expand (host): set96 = n_slots x (r_G | k_r_G), updated IN PLACE to the state after the last block; indices n_blocks x ell;
 * posts96 n_blocks x ell x (r_G | k_r_G).  out_instances: the n_blocks x 4 ell x 48 bytes cg1_shuffle_gather_points reads (vec_R | vec_S |
 * vec_T | vec_U).  out_plan: one entry per pre position (n_blocks x 2 ell: vec_R, then vec_S) saying where its decoded record already is --
 * >= 0: a point of the batch's own array, the T (U) position t of the earlier block b at b * stride_points + 2 ell + t (3 ell + t);
 * < 0: ~(set point index), the set holding r_G of slot s at point 2 s and k_r_G at 2 s + 1, as the set was before the call.
 * out_writers: (slot, writer) for every slot the blocks wrote, slots ascending, writer = b * ell + t of the slot's last write (room for
 * min(n_slots, n_blocks * ell) pairs), *out_n_writers their number.  Each output may be NULL.  An index >= n_slots: CG1_ERR_ARG, and nothing
 * is written, set96 included.
 * cg1_batch_decompress_strided_enqueue: cg1_batch_decompress_enqueue (unchecked) through an index map -- of every group of `stride` points
 * the points [skip, skip + take) are decoded; the other positions of the three arrays are neither read nor written.
 * cg1_chain_gather_enqueue: for the groups [first_group, first_group + n_groups) of d_pts96 / d_pstat (n_points records of 96 bytes / status
 * bytes), point p < take of group g <- the record plan[(g - first_group) * take + p] names (as out_plan above).  A source >= 0 must lie in
 * an earlier group, at a position >= take: a decoded position, never a gathered one.
 * cg1_chain_scatter_enqueue: set point pairs[2 j] <- point pairs[2 j + 1] of d_pts96 / d_pstat; the set points of a call are distinct.
 * The three device entries check every index on the host (CG1_ERR_ARG, nothing launched), carry `plan` / `pairs` (host memory) through the
 * context's kept staging, launch on the context's stream and wait for nothing; record arrays are 16-byte aligned. */
int cg1_chain_expand(uint8_t* set96, size_t n_slots, const uint32_t* indices, const uint8_t* posts96, size_t n_blocks, size_t ell, size_t stride_points,
                     uint8_t* out_instances, int32_t* out_plan, uint32_t* out_writers, size_t* out_n_writers);
int cg1_batch_decompress_strided_enqueue(cg1_ctx* ctx, const void* d_in48, void* d_out_affine96, void* d_status, size_t n_groups, size_t stride,
                                         size_t skip, size_t take);
int cg1_chain_gather_enqueue(cg1_ctx* ctx, void* d_pts96, void* d_pstat, size_t n_points, const void* d_set_pts96, const void* d_set_pstat, size_t n_set_points,
                             const int32_t* plan, size_t first_group, size_t n_groups, size_t stride, size_t take);
int cg1_chain_scatter_enqueue(cg1_ctx* ctx, const void* d_pts96, const void* d_pstat, size_t n_points, void* d_set_pts96, void* d_set_pstat, size_t n_set_points,
                              const uint32_t* pairs, size_t n_pairs);
/* fold cg1_batch_decompress_device's per-point status bytes (n_proofs x points_per_proof) into status[]: a proof
 * with an undecodable point becomes CG1_SHUFFLE_BAD_POINT and its scalars are zeroed (BufReader.read_g1, util.py:143-147) */
int cg1_shuffle_apply_point_status(int32_t* status, const uint8_t* point_status, size_t n_proofs, size_t points_per_proof,
                                   uint8_t* scalars32, uint8_t* crs_scalars32, size_t ncrs);
/* out[j] = sum over proofs i with status[i] == 0 (status may be NULL = all) of crs_scalars[i][j]  (mod r) */
int cg1_shuffle_sum_crs_scalars(const uint8_t* crs_scalars32, const int32_t* status, size_t n_proofs, size_t ncrs, uint8_t* out32);

/* Whisk tracker-opening proofs in batches: IsValidWhiskOpeningProof (whisk_interface.py:147-169) ->
 * TrackerOpeningProof.verify (opening.py:60-79), wire format opening.py:94-106.  Own points per proof, in order:
 * k_G, k_r_G, r_G, A, B (5 encodings / 5 scalars); out_g_scalars32 holds each proof's scalar on the generator G
 * (add them up with cg1_shuffle_sum_crs_scalars(..., ncrs = 1)).  status: 0 or CG1_SHUFFLE_BAD_SCALAR / _BAD_WEIGHT;
 * undecodable points are found by cg1_batch_decompress_device (apply with cg1_shuffle_apply_point_status, 5 points per proof). */
int cg1_opening_prepare(size_t n, const uint8_t* trackers96 /* r_G | k_r_G */, const uint8_t* k_commitments48, const uint8_t* proofs128,
                        const uint8_t* weights /* n x 2 x scalar32 */, uint8_t* out_points48, uint8_t* out_scalars32,
                        uint8_t* out_g_scalars32, int32_t* status);

/* The same front-end on the device (csrc/kernels_opening.h; replaces the per-proof host work of opening.py:60-71 -- the transcript --
 * and of opening.py:73-74 as one random combination): host wire bytes in, d_points96 ((5 n + 1) x 96 B: the own points decoded WITH the
 * subgroup test, then the generator) and d_scalars32 ((5 n + 1) x 32 B, the last one the summed generator scalar) left on the device for
 * cg1_msm_device.  status[n]: 0 or CG1_SHUFFLE_BAD_SCALAR / _BAD_WEIGHT / _BAD_POINT (scalars of such a proof are zero); point_status[5 n]:
 * k_batch_decompress's codes (CG1_ERR_NOT_IN_SUBGROUP marks the proofs the exact check cg1_opening_exact decides);
 * out_g_scalars32 (n x 32 B, may be NULL): each proof's own generator scalar, for the culprit search.  No weight in the reference: it
 * asserts both equalities per proof; the random combination is the batch verifier's own. */
int cg1_opening_prepare_device(cg1_ctx* ctx, size_t n, const uint8_t* trackers96 /* r_G | k_r_G */, const uint8_t* k_commitments48,
                               const uint8_t* proofs128, const uint8_t* weights /* n x 2 x scalar32, or NULL */, const uint8_t* seed32 /* used when weights == NULL */,
                               void* d_points96, void* d_scalars32, int32_t* status, uint8_t* point_status, uint8_t* out_g_scalars32);
/* The weights both front-ends use when the caller supplies none: proof i gets rho1 | rho2 = two 128-bit values (as scalar32) from the first
 * 32 bytes of SHAKE256(seed32 || le64(i)); seed32 = 32 fresh bytes from the OS per batch.  Writes proofs first .. first + n - 1. */
int cg1_opening_weights_from_seed(const uint8_t seed32[32], size_t first, size_t n, uint8_t* out_weights64);

/* Whisk tracker-opening proofs, the PROVER: GenerateWhiskTrackerProof (whisk_interface.py:177-190) -> TrackerOpeningProof.new
 * (opening.py:33-56) for n items (tracker, k, blinder b): decode k_r_G and r_G unchecked (a point outside G1 is multiplied exactly),
 * k_G = k G, A = b G, B = b r_G, the six appends [k_G, G, k_r_G, r_G, A, B] re-serialised and the challenge c, s = b - c k.
 * out_proofs128[i] = A | B | s (opening.py:94-99), out_k_commitments48[i] = k_G (the caller's k_commitment).  status[i]: 0, or
 * CG1_SHUFFLE_BAD_POINT (k_r_G or r_G does not decode: the reference raises ValueError before it draws a blinder), CG1_SHUFFLE_BAD_SCALAR
 * (k >= r), CG1_OPENING_BAD_BLINDER (b == 0 or b >= r), checked in that order; a rejected item gets a zeroed proof and k_commitment.
 * The k_r_G = k r_G relation is not checked (the reference does not check it either).
 * Host: on the worker pool (what a few proofs should take: a GPU round trip costs more than their scalar multiplications). */
#define CG1_OPENING_BAD_BLINDER  4   /* = CG1_SHUFFLE_BAD_WEIGHT: a blinder that is zero or >= r */
int cg1_opening_prove(size_t n, const uint8_t* trackers96 /* r_G | k_r_G */, const uint8_t* ks32, const uint8_t* blinders32,
                      uint8_t* out_proofs128, uint8_t* out_k_commitments48, int32_t* status);
/* The same proofs on the device (csrc/kernels_opening_prover.h), byte for byte and with the same status codes; host buffers in and out.
 * blinders32 == NULL: blinder i = int.from_bytes(SHAKE256("whisk_opening_blinder" || seed32 || le64(i)).digest(64), "little") mod r,
 * derived on the device.  A seed that is reused or known to anyone else reveals every k it was used with (k = (b - s) / c). */
int cg1_opening_prove_device(cg1_ctx* ctx, size_t n, const uint8_t* trackers96 /* r_G | k_r_G */, const uint8_t* ks32,
                             const uint8_t* blinders32 /* or NULL */, const uint8_t* seed32 /* used when blinders32 == NULL */,
                             uint8_t* out_proofs128, uint8_t* out_k_commitments48, int32_t* status);
/* Fixed-base multiples of the generator: out[i] = scalars[i] * G (any 256-bit scalar; k G = (k mod r) G) from a table of G built once per
 * context at the first call (csrc/kernels_generator.h: signed 8-bit windows, 32 mixed additions and one inversion per output against
 * k_batch_mul's 255 doublings).  Device pointers; d_out_affine96 (zeros = identity) and d_out48 (compressed) may each be NULL, not both. */
int cg1_generator_mul_device(cg1_ctx* ctx, const void* d_scalars32, size_t n, void* d_out_affine96 /* nullable */, void* d_out48 /* nullable */);

/* ---- Resident tables of FIXED bases, and MSMs over them without a doubling (csrc/kernels_fixed.h).
 * The bases the protocol's small MSMs run over never change (the CRS, crs.py:92-101).  A table holds, for every base B and every
 * window w = 0 .. 31, the 128 multiples d * 2^(8 w) * B as prepared records -- 512 KiB per base, built in one call for all bases
 * (the builder of the generator's table above) -- and a term k * B is then at most 32 additions of records picked by the signed
 * 8-bit digits of k.  The sum is finished on the device: no bucket reduction, no host Horner.
 *   cg1_fixed_create   n_bases = 1 .. CG1_FIXED_MAX_BASES (beyond, the table would pass 512 MiB: CG1_ERR_ARG).  A base is any point of
 *                      the CURVE (it need not lie in G1) or the all-zero identity record, whose entries are identities; a coordinate
 *                      >= p is CG1_ERR_ENCODING, a point off the curve CG1_ERR_NOT_ON_CURVE.  NULL on failure, the status in *status
 *                      (nullable).  The table lives on ctx's device and is used with contexts of that device; destroy it before them.
 *   cg1_fixed_msm      n_msm MSMs in one launch: MSM j sums term_scalars32[t] * base[term_base[t] & 0x7fffffff] over the terms
 *                      t = offsets[j] .. offsets[j + 1] - 1 (offsets[0] = 0; bit 31 of term_base[t] = the NEGATED base, cg1_lincomb_batch's
 *                      convention; an index may repeat).  An empty MSM is the identity.  Host buffers in and out; out_blobs144 and
 *                      out_comp48 may each be NULL, not both.  At most CG1_FIXED_MAX_MSMS MSMs per call and CG1_FIXED_MAX_TERMS terms
 *                      per MSM, an index outside the table: CG1_ERR_ARG.  A scalar >= r: CG1_ERR_ENCODING for the whole call, checked
 *                      before anything is written -- never reduced: outside G1 k P depends on k itself, not only on k mod r.
 *   cg1_fixed_msm_device   the same over DEVICE arrays (indices, scalars, n_msm + 1 offsets; n_terms = their length, max_terms >= the
 *                      longest MSM: both size the launch, and an MSM that exceeds them fails the call with CG1_ERR_ARG without reading
 *                      past the arrays).  Results stay on the device as affine96 (zeros = identity) and / or compressed48, enqueued on
 *                      the context's stream; the call returns once the status word is back.  A failed call writes no output.
 *   cg1_fixed_digits   host only, test support: the recoding k = sum_w out[w] 2^(8 w), |out[w]| <= 128, compiled from the function the
 *                      kernel runs (csrc/fixed_digits.h).  Meaningful for scalars below r. */
#define CG1_FIXED_MAX_BASES 1024
#define CG1_FIXED_MAX_MSMS  1024
#define CG1_FIXED_MAX_TERMS 2048
typedef struct cg1_fixed cg1_fixed;
cg1_fixed* cg1_fixed_create(cg1_ctx* ctx, const uint8_t* bases_affine96, size_t n_bases, int* status /* nullable */);
void   cg1_fixed_destroy(cg1_fixed* tab);
size_t cg1_fixed_len(const cg1_fixed* tab);
size_t cg1_fixed_bytes(const cg1_fixed* tab);                        /* device bytes of the table's records */
int cg1_fixed_msm(cg1_ctx* ctx, cg1_fixed* tab, const uint32_t* term_base, const uint8_t* term_scalars32, const uint32_t* offsets, size_t n_msm,
                  uint8_t* out_blobs144 /* nullable */, uint8_t* out_comp48 /* nullable */);
int cg1_fixed_msm_device(cg1_ctx* ctx, cg1_fixed* tab, const void* d_term_base, const void* d_term_scalars32, const void* d_offsets, size_t n_msm,
                         size_t n_terms, size_t max_terms, void* d_out_affine96 /* nullable */, void* d_out_comp48 /* nullable */);
void cg1_fixed_digits(const uint8_t scalar32[32], int16_t out[32]);

/* ---- The inner-product argument PROVED on the device: IPA.new (ipa.py:75-153) after its blinders are drawn, for n_provers independent
 * provers of one vector length n in step, as ONE launch chain with one host wait (csrc/kernels_ipa.h, csrc/ipa_rounds.h).
 * The bases stay what they are -- entries of a cg1_fixed table -- and the round challenges fold into the scalars: per round one
 * k_table_msm launch of 4 MSMs of n / 2 (+ 1) terms per prover, one k_fixed_finish (the encodings, on the device) and one k_ipa_step
 * (the transcript over the prover's own state, gamma^-1, the folds, the next round's scalars): 1 + 3 (lg n + 1) launches in all.
 *   per prover p, host buffers:
 *     g_index[p n ..], g_prime_index[p n ..]   table indices of crs_G_vec / crs_G_prime_vec;  h_index[p]  that of crs_H (crs_H * beta is
 *                         never formed: beta multiplies the inner-product scalars)
 *     g_prime_coeffs32    NULL, or n scalars per prover: entry j of G' stands for base * coeff (grand_prod.py:64-71 without a multiplication)
 *     cd48                C | D as 48-byte encodings.  They are only HASHED: validated (compression flag, x < p, on the curve; no
 *                         subgroup test) and absorbed re-serialised as the reference does (an identity as C0 00 .. 00)
 *     z32, vec_c32, vec_d32, vec_r_c32, vec_r_d32   canonical scalars; the blinders are the caller's (generate_ipa_blinders, ipa.py:27-48)
 *     states208           in: the transcript where IPA.new would find it; out: after the last ipa_gamma
 *     out_proofs          cg1_ipa_proof_bytes(n) = (2 + 4 lg n) 48 + 64 bytes each, IPA.to_bytes order:
 *                         B_c | B_d | vec_L_C | vec_R_C | vec_L_D | vec_R_D | c_final | d_final
 *     out_clocks          NULL, or 4 words per prover: clock ticks (s_memtime) of its lane 0 in the transcript | in the inversions of gamma | in the
 *                         whole of the steps that emit terms (all but the last) | steps counted
 *   The returned status covers the whole call, and a refused call leaves out_proofs and states208 untouched.  Refused before anything
 *   is written: n not a power of two in 2 .. CG1_IPA_MAX_N (the reference itself fails at n = 1; beyond, an MSM would pass
 *   CG1_FIXED_MAX_TERMS) or more than CG1_IPA_MAX_PROVERS provers (4 MSMs each per launch against CG1_FIXED_MAX_MSMS: larger batches
 *   are REFUSED, not chunked -- the caller splits them), an index outside the table, a table of another device: CG1_ERR_ARG; a scalar
 *   >= r: CG1_ERR_ENCODING (never reduced); an undecodable C or D: cg1_validate_compressed's status.
 *   cg1_ctx_set_param "ipa_inv" (0: binary Euclid, 1: a^(r-2)) picks the inversion of a round challenge -- an A/B switch, same bytes.
 *   cg1_ipa_round_emulate   host only, test support: the scalar schedule and the folds compiled from the header the kernel runs
 *                         (csrc/ipa_rounds.h).  State: c32 / d32 (len scalars, in and out), kg32 / kgp32 (n0 coefficients of the original
 *                         indices, in and out), kh32.  op 0: the step-1 terms (B_c over r_c32, B_d over r_d32 and kgp32; 2 MSMs, 3
 *                         offsets; len = n0).  op 1: c <- r_c + x c, d <- r_d + x d with x = challenge32 (alpha).  op 2: the round's terms
 *                         at the current length len (4 MSMs -- L_C, L_D, R_C, R_D --, 5 offsets, 2 n0 + 2 terms; out_term_base bit 31 =
 *                         the negated base, never set), then, when challenge32 (gamma) is not NULL, the fold: c32 / d32 hold len / 2
 *                         scalars afterwards.  The same refusals: CG1_ERR_ARG / CG1_ERR_ENCODING. */
#define CG1_IPA_MAX_N       2048
#define CG1_IPA_MAX_PROVERS 256
size_t cg1_ipa_proof_bytes(size_t n);                               /* 0 when n is not a power of two >= 2 */
int cg1_ipa_prove_device(cg1_ctx* ctx, cg1_fixed* tab, size_t n, size_t n_provers, const uint32_t* g_index, const uint32_t* g_prime_index,
                         const uint32_t* h_index, const uint8_t* g_prime_coeffs32 /* nullable */, const uint8_t* cd48, const uint8_t* z32,
                         const uint8_t* vec_c32, const uint8_t* vec_d32, const uint8_t* vec_r_c32, const uint8_t* vec_r_d32, uint8_t* states208,
                         uint8_t* out_proofs, uint32_t* out_clocks /* nullable */);
int cg1_ipa_round_emulate(int op, size_t n0, size_t len, uint8_t* c32, uint8_t* d32, uint8_t* kg32, uint8_t* kgp32, const uint8_t* kh32,
                          const uint8_t* challenge32 /* nullable for op 2 */, const uint8_t* r_c32, const uint8_t* r_d32, const uint32_t* g_index,
                          const uint32_t* g_prime_index, uint32_t h_index, uint32_t* out_term_base, uint8_t* out_term_scalars32, uint32_t* out_offsets);

/* ---- LIGHT tables: window multiples of VARIABLE bases, built on the device inside the call, and MSMs over them without a doubling
 * (csrc/kernels_light.h).  For bases that live for one proof and enter several MSMs each -- vec_T / vec_U of the same-MSM argument -- a
 * cg1_fixed table (512 KiB, ~0.35 ms per base) is unaffordable.  A light table uses signed windows of CG1_LIGHT_WINDOW_BITS = 4 bits:
 * per base 64 windows x 8 multiples d * 2^(4 w) * B as 256-byte XYZZ records (no inversion in the build), 128 KiB; a term k * B is then
 * at most 64 additions.  Built by two launches: one wave per base walks the 252 doublings, then one wave per (base, window) fills the
 * multiples; every addition is complete and every record carries its own identity flag, so the table is exact for ANY curve point.
 *   cg1_light_create   n_bases = 1 .. CG1_LIGHT_MAX_BASES; the coordinate and on-curve errors, the all-zero identity record and the
 *                      device rules of cg1_fixed_create.
 *   cg1_light_msm, cg1_light_msm_device   the arguments, outputs, limits and refusals of cg1_fixed_msm / cg1_fixed_msm_device (bit 31
 *                      of an index = the negated base; a scalar >= r: CG1_ERR_ENCODING for the whole call, never reduced; an index
 *                      outside the table or bad offsets: CG1_ERR_ARG; a refused call writes nothing), with CG1_LIGHT_MAX_MSMS and
 *                      CG1_LIGHT_MAX_TERMS in place of the fixed tables' limits.
 *   cg1_light_digits   host only, test support: the recoding k = sum_w out[w] 2^(CG1_LIGHT_WINDOW_BITS w), |out[w]| <= 2^(bits - 1),
 *                      compiled from the function the kernel runs (csrc/light_digits.h); writes and returns CG1_LIGHT_WINDOWS digits.
 *                      Meaningful for scalars below r.
 * Limits: CG1_LIGHT_MAX_BASES = 16 384 = 64 provers x 2 n bases at n = 128, the largest batch the prover's records hold; at 128 KiB each
 * that is 2 GiB of records.  CG1_LIGHT_MAX_MSMS and CG1_LIGHT_MAX_TERMS equal the fixed tables': the kernels share the ticket words (one
 * per MSM), the finishing kernel's records and the slices of at most 128 terms whose partial sums one workgroup joins.
 * CG1_LIGHT_WINDOW_BITS may be overridden when the library is built (3 .. 7; an A/B switch for the window plan: tools/gpu_light_table_timing.py). */
#ifndef CG1_LIGHT_WINDOW_BITS
#define CG1_LIGHT_WINDOW_BITS 4
#endif
#define CG1_LIGHT_WINDOWS ((256 + CG1_LIGHT_WINDOW_BITS - 1) / CG1_LIGHT_WINDOW_BITS)
#define CG1_LIGHT_MAX_BASES 16384
#define CG1_LIGHT_MAX_MSMS  1024
#define CG1_LIGHT_MAX_TERMS 2048
typedef struct cg1_light cg1_light;
cg1_light* cg1_light_create(cg1_ctx* ctx, const uint8_t* bases_affine96, size_t n_bases, int* status /* nullable */);
void   cg1_light_destroy(cg1_light* tab);
size_t cg1_light_len(const cg1_light* tab);
size_t cg1_light_bytes(const cg1_light* tab);                        /* device bytes of the table's records */
int cg1_light_msm(cg1_ctx* ctx, cg1_light* tab, const uint32_t* term_base, const uint8_t* term_scalars32, const uint32_t* offsets, size_t n_msm,
                  uint8_t* out_blobs144 /* nullable */, uint8_t* out_comp48 /* nullable */);
int cg1_light_msm_device(cg1_ctx* ctx, cg1_light* tab, const void* d_term_base, const void* d_term_scalars32, const void* d_offsets, size_t n_msm,
                         size_t n_terms, size_t max_terms, void* d_out_affine96 /* nullable */, void* d_out_comp48 /* nullable */);
int cg1_light_digits(const uint8_t scalar32[32], int16_t out[CG1_LIGHT_WINDOWS]);

/* ---- The same-MSM argument PROVED on the device: SameMSMProof.new (same_msm.py:50-143) after its generate_blinders(n) draw, for
 * n_provers independent provers of one length n in step, as ONE launch chain with one host wait (csrc/kernels_same_msm.h,
 * csrc/same_msm_rounds.h).  All bases stay what they are and the round challenges fold into the scalars through one coefficient vector
 * per prover.  crs_G_vec are entries of a cg1_fixed table; vec_T | vec_U are per-proof points: the call builds ONE light table over all
 * provers' T and U (scratch kept with the cg1_fixed handle, regrown only when too small).  Per step two MSM launches of k_table_msm -- the fixed plan for
 * the A side, the light plan for T and U --, their two k_fixed_finish and one k_smsm_step (the transcript over the prover's own state,
 * gamma^-1, the fold, the next terms): 3 + 5 (lg n + 1) launches in all.
 *   per prover p, host buffers:
 *     g_index[p n ..]     table indices of crs_G_vec
 *     azz48               A | Z_t | Z_u as 48-byte encodings.  They are only HASHED: validated (compression flag, x < p, on the curve; no
 *                         subgroup test) and absorbed re-serialised as the reference does (an identity as C0 00 .. 00)
 *     tu_affine96         vec_T | vec_U: 2 n affine96 records (all-zero = the identity); any curve point, nothing is decoded or subgroup-tested
 *     vec_x32, vec_r32    canonical scalars; vec_r is the caller's generate_blinders(n); vec_x is not written
 *     states208           in: the transcript where SameMSMProof.new would find it; out: after the last same_msm_gamma.  The first two
 *                         same_msm_step1 lists ([A, Z_t, Z_u]; vec_T + vec_U) depend on nothing the device computes and are absorbed on
 *                         the host into the states that are uploaded; the third list and everything after it on the device
 *     out_proofs          cg1_same_msm_proof_bytes(n) = (3 + 6 lg n) 48 + 32 bytes each, SameMSMProof.to_bytes order:
 *                         B_a | B_t | B_u | vec_L_A | vec_L_T | vec_L_U | vec_R_A | vec_R_T | vec_R_U | x_final
 *     out_clocks          NULL, or 4 words per prover, as cg1_ipa_prove_device
 *   The returned status covers the whole call, and a refused call leaves out_proofs and states208 untouched.  Refused before anything
 *   is written: n not a power of two in 2 .. CG1_SAME_MSM_MAX_N, more than CG1_SAME_MSM_MAX_PROVERS provers or n_provers 2 n >
 *   CG1_LIGHT_MAX_BASES (REFUSED, not chunked -- the caller splits), an index outside the table, a table of another device: CG1_ERR_ARG;
 *   a scalar >= r: CG1_ERR_ENCODING (never reduced); a T or U coordinate >= p or a point off the curve: cg1_from_affine96's status; an
 *   undecodable A, Z_t or Z_u: cg1_validate_compressed's status.
 * Limits: CG1_SAME_MSM_MAX_N = 1024: one prover's 2 n = 2048 light records are 256 MiB, and an MSM of step B has n terms <=
 * CG1_FIXED_MAX_TERMS.  CG1_SAME_MSM_MAX_PROVERS = 64: 64 provers x 2 n at n = 128 is CG1_LIGHT_MAX_BASES (2 GiB of records), and the 4
 * MSMs per prover of a launch over T | U stay within CG1_LIGHT_MAX_MSMS.
 *   cg1_same_msm_round_emulate   host only, test support: the scalar schedule and the fold compiled from the header the kernel runs
 *                         (csrc/same_msm_rounds.h).  State: x32 (len scalars, in and out), k32 (n0 coefficients, in and out).
 *                         op 0: the terms of step B over r32 (3 MSMs B_a, B_t, B_u; 4 offsets 0, n0, 2 n0, 3 n0; len = n0).
 *                         op 1: x <- r + a x with a = challenge32 (alpha).  op 2: the round's terms at the current length len (6 MSMs
 *                         in the transcript's order L_A, L_T, L_U, R_A, R_T, R_U; 7 offsets 0, h, .., 6 h with h = n0 / 2), then, when
 *                         challenge32 (gamma) is not NULL, the fold: x32 holds len / 2 scalars afterwards.  Indices of the A lists are
 *                         g_index's (the fixed table); those of the T and U lists are light-table indices, T[j] at j and U[j] at n0 + j.
 *                         The same refusals: CG1_ERR_ARG / CG1_ERR_ENCODING. */
#define CG1_SAME_MSM_MAX_N       1024
#define CG1_SAME_MSM_MAX_PROVERS 64
size_t cg1_same_msm_proof_bytes(size_t n);                          /* 0 when n is not a power of two >= 2 */
int cg1_same_msm_prove_device(cg1_ctx* ctx, cg1_fixed* tab, size_t n, size_t n_provers, const uint32_t* g_index, const uint8_t* azz48,
                              const uint8_t* tu_affine96, const uint8_t* vec_x32, const uint8_t* vec_r32, uint8_t* states208, uint8_t* out_proofs,
                              uint32_t* out_clocks /* nullable */);
int cg1_same_msm_round_emulate(int op, size_t n0, size_t len, uint8_t* x32, uint8_t* k32, const uint8_t* challenge32 /* nullable for op 2 */,
                               const uint8_t* r32, const uint32_t* g_index, uint32_t* out_term_base, uint8_t* out_term_scalars32, uint32_t* out_offsets);

/* ---- The grand-product argument PROVED on the device: GrandProductProof.new (grand_prod.py:29-119) after its random draws, for n_provers
 * independent provers of one shape (ell, n_blinders; n = ell + n_blinders) in step, as ONE launch chain with one host wait
 * (csrc/kernels_gprod.h, csrc/gprod_rounds.h, then the phases of csrc/kernels_ipa.h).  vec_G = crs_G_vec | crs_H_vec are n entries of a
 * cg1_fixed table and never move: C = MSM(vec_G, c | c_blinders) over the prefix products c; the base change G'_i = G_i beta^-(i+1) is a
 * coefficient vector (the g_prime_coeffs32 of cg1_ipa_prove_device, made on the device), and D, which the reference builds from B, is the
 * MSM its own assertion says it is (grand_prod.py:105): D = MSM(vec_G, b_j - beta^-1 | r_b_j + alpha).  k_gprod_step begin | MSM finish |
 * k_gprod_step step (both transcript steps, the prefix products and powers by one workgroup scan, the completion of the IPA's blinders) |
 * MSM finish | the IPA's step 1 and lg n rounds: 1 + 3 (lg n + 2) launches.
 *   per prover p, host buffers:
 *     g_index[p n ..]     table indices of crs_G_vec | crs_H_vec;  u_index[p]  that of crs_U
 *     b48                 B as a 48-byte encoding: validated like cd48 above and hashed re-serialised.  The reference's assertions
 *                         (grand_prod.py:103-105) hold exactly when B = MSM(vec_G, vec_b | vec_b_blinders) and gprod_result is the product
 *                         of vec_b: the chain computes that MSM next to C, compares the encodings, compares the product, and REFUSES the
 *                         call where the reference raises AssertionError
 *     gprod_result32, vec_b32 (n scalars: vec_b | vec_b_blinders), vec_c_blinders32 (n_blinders)   canonical scalars
 *     ipa_r32 (n), ipa_z_head32 (n - 2)   the draws of generate_ipa_blinders (ipa.py:30-31) in its order; the device completes z with
 *                         penultimate_z, last_z (ipa.py:33-41; one inversion for both denominators)
 *     states208           in: the transcript where GrandProductProof.new would find it; out: after the last ipa_gamma
 *     out_proofs          cg1_gprod_proof_bytes(ell, n_blinders) = 48 + 32 + cg1_ipa_proof_bytes(n) bytes each, GrandProductProof.to_bytes
 *                         order: C | r_p | the IPA's proof
 *     out_clocks          NULL, or 4 words per prover, as cg1_ipa_prove_device (the inversions: beta, the blinders' and the gammas)
 *   The returned status covers the whole call, and a refused call leaves out_proofs and states208 untouched.  Refused before anything is
 *   written, in cg1_ipa_prove_device's order: n not a power of two in 2 .. CG1_IPA_MAX_N, ell < 1 or n_blinders < 2 (so n >= 4), more than
 *   CG1_IPA_MAX_PROVERS provers, an index outside the table, a table of another device: CG1_ERR_ARG; a scalar >= r: CG1_ERR_ENCODING (never
 *   reduced); an undecodable B: cg1_validate_compressed's status; vec_c_blinders[n_blinders - 2] = 0 (generate_ipa_blinders divides by it):
 *   CG1_ERR_ARG.  Refused at the chain's end, from its status word (CG1_GPROD_*; never a trap: a zero is tested BEFORE every inversion and
 *   the chain runs on with zeros): B not the commitment, gprod_result not the product, gprod_beta = 0, the second denominator of
 *   generate_ipa_blinders = 0 (r[n-1] c[n-2] = r[n-2] c[n-1]: draw ipa_r again): CG1_ERR_ARG, each with its own text.
 *   cg1_gprod_emulate     host only, test support: the formulas, the blinder completion and the term schedule compiled from the header the
 *                         kernel runs (csrc/gprod_rounds.h), with the two challenges given.  out_state32: 4 n scalars c | d | kGp | the
 *                         completed z;  out_scalars32: r_p | inner_prod;  the terms of the five MSMs B', C, D, B_c, B_d (5 n terms, 6
 *                         offsets 0, n, .., 5 n).  The same refusals by shape and encoding; for the others CG1_ERR_ARG with *out_status =
 *                         the CG1_GPROD_* bits (B is not looked at: evaluate the first term list). */
#define CG1_GPROD_BAD_COMMITMENT   0x100
#define CG1_GPROD_BAD_PRODUCT      0x200
#define CG1_GPROD_ZERO_BETA        0x400
#define CG1_GPROD_ZERO_C           0x800
#define CG1_GPROD_ZERO_DENOMINATOR 0x1000
size_t cg1_gprod_proof_bytes(size_t ell, size_t n_blinders);        /* 0 when ell < 1, n_blinders < 2 or ell + n_blinders is not a power of two */
int cg1_gprod_prove_device(cg1_ctx* ctx, cg1_fixed* tab, size_t ell, size_t n_blinders, size_t n_provers, const uint32_t* g_index, const uint32_t* u_index,
                           const uint8_t* b48, const uint8_t* gprod_result32, const uint8_t* vec_b32, const uint8_t* vec_c_blinders32,
                           const uint8_t* ipa_r32, const uint8_t* ipa_z_head32, uint8_t* states208, uint8_t* out_proofs, uint32_t* out_clocks /* nullable */);
int cg1_gprod_emulate(size_t ell, size_t n_blinders, const uint8_t* gprod_result32, const uint8_t* vec_b32, const uint8_t* vec_c_blinders32,
                      const uint8_t* ipa_r32, const uint8_t* ipa_z_head32, const uint8_t* alpha32, const uint8_t* beta32, const uint32_t* g_index,
                      uint8_t* out_state32, uint8_t* out_scalars32, uint32_t* out_term_base, uint8_t* out_term_scalars32, uint32_t* out_offsets,
                      uint32_t* out_status);

/* ---- The same-permutation argument PROVED on the device: SamePermutationProof.new (same_perm.py:27-72) after its callee's random draws,
 * for n_provers independent provers of one shape in step: the grand-product launch chain above with another head, still 1 + 3 (lg n + 2)
 * launches and one host wait (csrc/kernels_same_perm.h, csrc/same_perm_rounds.h, then k_gprod_step's step phase and the IPA's phases).
 * The bases never move.  With b_i = vec_a[perm[i]] + perm[i] alpha + beta and b_blinder_k = vec_a_blinders[k] + alpha vec_m_blinders[k], the
 * reference's B = A + alpha M + beta sum G_i equals B' = MSM(vec_G, b | b_blinders) exactly when A - A' + alpha (M - M') = O for
 * A' = MSM(vec_G, vec_a o perm | vec_a_blinders), M' = MSM(vec_G, perm | vec_m_blinders) -- which is also exactly when the reference's
 * assertion grand_prod.py:105 holds.  The first MSM launch computes A', M', B' and C (4 MSMs of n terms per prover); the chain compares the
 * encodings of A' and M' with the caller's A and M, REFUSES the call on a mismatch where the reference raises AssertionError, and EMITS B'
 * as B.  A = A' and M = M' is stricter than the reference's condition only on the event A - A' = -alpha (M - M') != O; alpha is drawn after
 * A and M are absorbed, so that event has negligible probability.  No point outside the table enters an MSM.
 * same_perm_step1 [A, M], same_perm_step1 vec_a and the challenges same_perm_alpha, same_perm_beta depend on nothing the device computes:
 * the entry runs them on the host, on the copy of the states it uploads, and uploads alpha and beta.
 *   per prover p, host buffers (g_index, u_index, vec_c_blinders32, ipa_r32, ipa_z_head32, states208, out_clocks: as cg1_gprod_prove_device):
 *     am48                A | M as 48-byte encodings: validated like b48 above and hashed re-serialised
 *     vec_a32 (ell), vec_a_blinders32, vec_m_blinders32 (n_blinders each)   canonical scalars
 *     perm                ell uint32 entries < ell; NOT required to be a bijection (the reference does not require it either)
 *     out_proofs          cg1_same_perm_proof_bytes(ell, n_blinders) = 48 + cg1_gprod_proof_bytes(ell, n_blinders) bytes each,
 *                         SamePermutationProof.to_bytes order: B | C | r_p | the IPA's proof
 *   Refusals as cg1_gprod_prove_device's, in its order, and: a perm entry >= ell (the reference's get_permutation raises IndexError):
 *   CG1_ERR_ARG; an undecodable A or M: cg1_validate_compressed's status; every scalar array is checked < r.  At the chain's end, from its
 *   status word: A or M not the commitment (CG1_SAME_PERM_*), then the grand-product chain's own (CG1_GPROD_*), each with its own text.  A
 *   refused call leaves out_proofs and states208 untouched.
 *   cg1_same_perm_emulate   host only, test support: the host transcript head and the formulas and term schedule compiled from the header
 *                         the kernel runs (csrc/same_perm_rounds.h).  state208: in/out, advanced past same_perm_beta (untouched by a refused
 *                         call);  out_challenges32: alpha | beta;  out_b32: n scalars b | b_blinders;  out_gprod_result32;  the terms of
 *                         the four MSMs A', M', B', C (4 n terms, 5 offsets 0, n, .., 4 n; vec_c_blinders32 is what C's list ends in).  The
 *                         entry's refusals by shape, permutation and encoding; *out_status = 0 (A and M are only decoded: evaluate the
 *                         first two term lists). */
#define CG1_SAME_PERM_BAD_A        0x2000
#define CG1_SAME_PERM_BAD_M        0x4000
size_t cg1_same_perm_proof_bytes(size_t ell, size_t n_blinders);    /* 0 when cg1_gprod_proof_bytes is */
int cg1_same_perm_prove_device(cg1_ctx* ctx, cg1_fixed* tab, size_t ell, size_t n_blinders, size_t n_provers, const uint32_t* g_index, const uint32_t* u_index,
                               const uint8_t* am48, const uint8_t* vec_a32, const uint32_t* perm, const uint8_t* vec_a_blinders32, const uint8_t* vec_m_blinders32,
                               const uint8_t* vec_c_blinders32, const uint8_t* ipa_r32, const uint8_t* ipa_z_head32, uint8_t* states208, uint8_t* out_proofs,
                               uint32_t* out_clocks /* nullable */);
int cg1_same_perm_emulate(size_t ell, size_t n_blinders, uint8_t* state208, const uint8_t* a48, const uint8_t* m48, const uint8_t* vec_a32, const uint32_t* perm,
                          const uint8_t* vec_a_blinders32, const uint8_t* vec_m_blinders32, const uint8_t* vec_c_blinders32, const uint32_t* g_index,
                          uint8_t* out_challenges32, uint8_t* out_b32, uint8_t* out_gprod_result32, uint32_t* out_term_base, uint8_t* out_term_scalars32,
                          uint32_t* out_offsets, uint32_t* out_status);

/* ---- The shuffle prover's same-scalar block PROVED on the device: what CurdleProofsProof.new runs between SamePermutationProof.new and
 * SameMSMProof.new (curdleproofs.py:92-116) -- R = MSM(vec_R, vec_a), S = MSM(vec_S, vec_a), cm_T = GroupCommitment.new(G_t, H, R k, r_t),
 * cm_U = GroupCommitment.new(G_u, H, S k, r_u) and all of SameScalarProof.new (same_scalar.py:39-69) after its three draws -- for n_provers
 * independent provers of one ell in step, as ONE launch chain with one host wait (csrc/kernels_same_scalar.h, csrc/same_scalar_rounds.h).
 * No base is ever multiplied on its own: R k = sum (k a_i) R_i and R r_k = sum (r_k a_i) R_i, so each of the ten points the block emits is an
 * MSM over G_t | G_u | H | vec_R | vec_S.  The call builds ONE light table of 3 + n_provers 2 ell bases (the scratch kept with the cg1_fixed
 * handle, shared with cg1_same_msm_prove_device and regrown only when too small; `tab` is the chain's home -- staging block, scratch, lock
 * -- and G_t, G_u, H need not be among its bases) and runs ONE k_table_msm launch of 10 MSMs per prover, ONE k_fixed_finish and
 * k_sscalar_step on both sides: upload | begin | the table's two build launches | [k_subgroup_row] | MSMs | finish | step: 6 launches, 7
 * with the subgroup test.
 *   sum (k a_i mod r) R_i = k (sum a_i R_i) holds only for bases of order r, and nothing here decodes or tests a point on the host:
 *     bases_certified     0: the chain tests every vec_R | vec_S record on the device (k_subgroup_row; the all-zero identity record is in
 *                         G1) and a record outside G1 REFUSES the call at its end: CG1_ERR_NOT_IN_SUBGROUP with its own text, status bit
 *                         CG1_SAME_SCALAR_NOT_G1 of the chain's word -- never a trap, never wrong bytes.  1: the caller vouches that every
 *                         record lies in G1 and the launch is skipped.
 *   host buffers:
 *     gth_affine96        G_t | G_u | H: three affine96 records, shared by all provers (any curve points)
 *     rs_affine96         per prover vec_R | vec_S: 2 ell affine96 records (all-zero = the identity)
 *     vec_a32 (ell per prover), k32 (1), blinders32 (5: r_t r_u r_a r_b r_k)   canonical scalars; the draws are the caller's, in the
 *                         reference's order (r_t, r_u at curdleproofs.py:92-93, then r_a, r_b, r_k at same_scalar.py:39-41)
 *     states208           in: the transcript where the block would find it; out: after same_scalar_alpha
 *     out_proofs          cg1_same_scalar_proof_bytes() = 576 bytes each: cm_T | cm_U | R | S | cm_A | cm_B | z_k | z_t | z_u, a commitment
 *                         as T_1 | T_2 -- CurdleProofsProof.to_bytes order without A, M and the other two arguments' proofs
 *     out_clocks          NULL, or 4 words per prover: clock ticks of its lane 0 in the transcript | 0 | 0 | transcript programs run (2)
 *   The returned status covers the whole call, and a refused call leaves out_proofs and states208 untouched.  Refused before anything is
 *   written: a null pointer or a table of another device, ell outside 1 .. CG1_SAME_SCALAR_MAX_ELL (ell need not be a power of two), more
 *   than CG1_SAME_SCALAR_MAX_PROVERS provers or 3 + n_provers 2 ell > CG1_LIGHT_MAX_BASES (REFUSED, not chunked -- the caller splits):
 *   CG1_ERR_ARG; a scalar >= r: CG1_ERR_ENCODING (never reduced); a coordinate >= p or a point off the curve: cg1_from_affine96's status,
 *   the text naming the prover and the entry.
 * Limits: CG1_SAME_SCALAR_MAX_ELL = 1024: an MSM has ell + 1 terms <= CG1_LIGHT_MAX_TERMS and one prover's 2 ell light records are 256 MiB.
 * CG1_SAME_SCALAR_MAX_PROVERS = 64: 10 MSMs per prover within CG1_LIGHT_MAX_MSMS, and 3 + 64 x 2 ell bases at ell = 124 fit the table.
 *   cg1_same_scalar_emulate   host only, test support: the term schedule and the formulas compiled from the header the kernel runs
 *                         (csrc/same_scalar_rounds.h), one prover whose vec_R starts at light-table index 3.  The terms of the ten MSMs in
 *                         the transcript's order R, S, T.T_1, T.T_2, U.T_1, U.T_2, A.T_1, A.T_2, B.T_1, B.T_2 (6 ell + 8 terms, 11 offsets).
 *                         With enc480 (the ten 48-byte encodings, validated like cd48 above) also the transcript step on state208 (in /
 *                         out; untouched by a refused call): out_alpha32 and out_z96 = z_k | z_t | z_u.  enc480 NULL: state208, out_alpha32
 *                         and out_z96 are not looked at.  The entry's refusals by shape and encoding. */
#define CG1_SAME_SCALAR_NOT_G1     0x8000
#define CG1_SAME_SCALAR_MAX_ELL     1024
#define CG1_SAME_SCALAR_MAX_PROVERS 64
size_t cg1_same_scalar_proof_bytes(void);                           /* 576 */
int cg1_same_scalar_prove_device(cg1_ctx* ctx, cg1_fixed* tab, size_t ell, size_t n_provers, const uint8_t* gth_affine96, const uint8_t* rs_affine96,
                                 const uint8_t* vec_a32, const uint8_t* k32, const uint8_t* blinders32 /* r_t r_u r_a r_b r_k per prover */,
                                 int bases_certified, uint8_t* states208, uint8_t* out_proofs, uint32_t* out_clocks /* nullable */);
int cg1_same_scalar_emulate(size_t ell, const uint8_t* vec_a32, const uint8_t* k32, const uint8_t* blinders32, const uint8_t* enc480 /* nullable */,
                            uint8_t* state208 /* nullable with enc480 */, uint32_t* out_term_base, uint8_t* out_term_scalars32, uint32_t* out_offsets,
                            uint8_t* out_alpha32, uint8_t* out_z96);

/* ---- A whole shuffle proof PROVED on the device: CurdleProofsProof.new (curdleproofs.py:63-160) for n_provers shuffles of one ell in
 * step, as ONE native call -- instances, permutations, k and the draws in, n_provers times CurdleProofsProof.to_bytes() out.  N_BLINDERS = 4
 * is fixed; n = ell + 4 is a power of two in 8 .. CG1_SAME_MSM_MAX_N; n_provers <= CG1_SAME_MSM_MAX_PROVERS and n_provers 2 n <=
 * CG1_LIGHT_MAX_BASES (64 provers at ell = 124).  The call creates the `curdleproofs` transcript itself; it takes none.
 * The pipeline (csrc/capi_shuffle.h; one stream, two event waits and the stream wait at its end):
 *   host     curdleproofs_step1 [vec_R + vec_S + vec_T + vec_U], M, the ell challenges curdleproofs_vec_a -- per prover, on the process's
 *            worker pool
 *   device   k_shuffle_begin (csrc/kernels_shuffle.h, csrc/shuffle_rounds.h): the terms of A and A', vec_x, the terms of the same-scalar
 *            block's ten MSMs; then A = MSM(vec_G | vec_H, a o perm | a_blinders | 0 | 0) and A' = MSM(vec_G | vec_H[:2] | G_t | G_u,
 *            a o perm | a_blinders | r_t | r_u) = A + cm_T.T_1 + cm_U.T_1 as ONE k_table_msm launch; then, without a wait, the
 *            same-scalar block's light table and MSMs
 *   host     (first wait: A) the same-permutation head; device: its chain (cg1_same_perm_prove_device's), then the same-scalar block's step
 *            on the states that chain left; then, without a wait, the same-MSM chain's begin and its light table over
 *            vec_T | O O H O | vec_U | O O O H
 *   host     (second wait: cm_T, cm_U) same_msm_step1 [A', Z_t, Z_u] and the 2 n encodings; device: the rest of the same-MSM chain
 *   per prover p, host buffers:
 *     g_index (ell), h_index (4), u_index, gt_index, gu_index (1 each)   table indices of crs.vec_G, crs.vec_H, crs.H, crs.G_t, crs.G_u
 *     gth_affine96        G_t | G_u | H: three affine96 records, shared by all provers
 *     rs_affine96, tu_affine96   per prover vec_R | vec_S and vec_T | vec_U: 2 ell affine96 records each (all-zero = the identity)
 *     m48                 M, 48 bytes; perm: ell entries < ell (not required to be a bijection); k32: the scalar k
 *     vec_m_blinders32 (4)   the blinders of M;  the draws, in the reference's order:  vec_a_blinders32 (2) | vec_c_blinders32 (4),
 *     ipa_r32 (n), ipa_z_head32 (n - 2) as cg1_same_perm_prove_device takes them | blinders32 (5: r_t r_u r_a r_b r_k) | vec_r32 (n)
 *     bases_certified     as cg1_same_scalar_prove_device's: 1 only when every vec_R | vec_S record is known to lie in G1
 *     out_proofs          cg1_shuffle_prover_proof_bytes(ell) bytes each: A | cm_T | cm_U | R | S | same_perm | cm_A | cm_B | z_k | z_t | z_u |
 *                         same_msm -- the verifier's wire proof (cg1_shuffle_proof_bytes of a CRS handle) without its leading M
 *     out_clocks          NULL, or 4 words per prover: the three chains' clock words, summed
 *   The returned status covers the whole call, and a refused call leaves out_proofs untouched.  The refusals are those of the three
 *   entries above, run on the arguments they see, each text with this entry's name: CG1_ERR_ARG for a shape, a null pointer, an index
 *   outside the table, a perm entry >= ell, an M that is not the commitment to perm | vec_m_blinders (CG1_SAME_PERM_BAD_M) and the
 *   grand-product chain's own; CG1_ERR_ENCODING for a scalar >= r; cg1_from_affine96's / cg1_validate_compressed's status for a point;
 *   CG1_ERR_NOT_IN_SUBGROUP for a vec_R | vec_S record outside G1.
 *   cg1_shuffle_begin_emulate   host only, test support: the formulas and term schedule compiled from the header k_shuffle_begin runs, one
 *                         prover, any ell in 1 .. CG1_SAME_SCALAR_MAX_ELL: the 2 n terms of A | A' (3 offsets), vec_x (n), and the same-scalar
 *                         block's 6 ell + 8 terms (11 offsets) as cg1_same_scalar_emulate lays them out.  A perm entry >= ell: CG1_ERR_ARG. */
size_t cg1_shuffle_prover_proof_bytes(size_t ell);                  /* 0 when ell + 4 is not a power of two in 8 .. CG1_SAME_MSM_MAX_N */
int cg1_shuffle_prove_device(cg1_ctx* ctx, cg1_fixed* tab, size_t ell, size_t n_provers, const uint32_t* g_index, const uint32_t* h_index, const uint32_t* u_index,
                             const uint32_t* gt_index, const uint32_t* gu_index, const uint8_t* gth_affine96, const uint8_t* rs_affine96, const uint8_t* tu_affine96,
                             const uint8_t* m48, const uint32_t* perm, const uint8_t* k32, const uint8_t* vec_m_blinders32, const uint8_t* vec_a_blinders32,
                             const uint8_t* vec_c_blinders32, const uint8_t* ipa_r32, const uint8_t* ipa_z_head32, const uint8_t* blinders32, const uint8_t* vec_r32,
                             int bases_certified, uint8_t* out_proofs, uint32_t* out_clocks /* nullable */);
int cg1_shuffle_begin_emulate(size_t ell, const uint8_t* vec_a32, const uint32_t* perm, const uint8_t* k32, const uint8_t* blinders32 /* r_t r_u r_a r_b r_k */,
                              const uint8_t* vec_a_blinders32 /* 2 */, const uint32_t* gi_a, const uint32_t* gi_m, uint32_t* out_term_base, uint8_t* out_term_scalars32,
                              uint32_t* out_offsets, uint8_t* out_vec_x32, uint32_t* out_ss_term_base, uint8_t* out_ss_term_scalars32, uint32_t* out_ss_offsets);

/* ---- GenerateWhiskShuffleProof (whisk_interface.py:111-140) from tracker BYTES, for n_provers shuffles of one ell in step: pre-shuffle
 * trackers, permutations, k and the draws in; post-shuffle tracker bytes and M || proof out.  The limits are cg1_shuffle_prove_device's.
 * cg1_whisk_shuffle_front (csrc/capi_whisk_shuffle.h, csrc/kernels_whisk_shuffle.h) is everything in front of CurdleProofsProof.new, on
 * the context's stream with one wait at its end:
 *   k_table_msm + k_fixed_finish   M = MSM(vec_G | vec_H, perm | vec_m_blinders) of every prover as one launch over the CRS table
 *   k_batch_decompress_row         the n_provers 2 ell encodings -> affine96 (its leniency: the infinity flag wins over the other bits)
 *   k_subgroup_row, k_whisk_status the G1 certificate of every decoded point, folded with the decoder's status into one word per call
 *   k_whisk_permute_mul            one wave per output: T_i = k R_perm[i], U_i = k S_perm[i], affine96 and the 48-byte encoding
 *   per prover p, host buffers:
 *     g_index (ell), h_index (4)   table indices of crs.vec_G and crs.vec_H
 *     trackers96          ell records r_G48 | k_r_G48 (cg1_opening_prove's layout): R_i = r_G of tracker i, S_i = its k_r_G
 *     perm                ell entries < ell (not required to be a bijection); k32; vec_m_blinders32 (4)
 *     out_rs_affine96, out_tu_affine96   vec_R | vec_S and vec_T | vec_U, 2 ell affine96 records each, as cg1_shuffle_prove_device takes them
 *     out_post96          ell records T_i48 | U_i48: the post-shuffle trackers;  out_m48: M
 *   Refusals: a status for the whole call, the text (cg1_ctx_error) starting with the entry's name and, for a point, naming the prover, the
 *   tracker index and the half (r_G / k_r_G); a refused call leaves every output untouched.  CG1_ERR_ARG: a null pointer, a table of
 *   another device, ell + 4 not a power of two in 8 .. CG1_SAME_MSM_MAX_N, n_provers beyond cg1_shuffle_prove_device's limits, an index
 *   outside the table, a perm entry >= ell.  CG1_ERR_ENCODING: k or a blinder >= r, an encoding without the compression flag or with
 *   x >= p.  CG1_ERR_NOT_ON_CURVE.  CG1_ERR_NOT_IN_SUBGROUP: a tracker point outside G1 -- the reference would go on with it
 *   (util.py:35-36 decodes unchecked); here k folds into the same-scalar block's scalars, which is exact only in G1.
 * cg1_whisk_shuffle_prove_device   the front, then cg1_shuffle_prove_device on its vec_R | vec_S, vec_T | vec_U and M with bases_certified
 *   = 1, in one native call; the remaining arguments are cg1_shuffle_prove_device's.  out_proofs: cg1_whisk_shuffle_proof_bytes(ell) = 48 +
 *   cg1_shuffle_prover_proof_bytes(ell) bytes per prover, M || proof: the wire form cg1_shuffle_proof_bytes(crs) counts.  A refusal of
 *   either half leaves out_post96 and out_proofs untouched; the chain's texts come back under this entry's name.
 * cg1_whisk_shuffle_front_emulate   host only, test support: the front for ONE prover over the host's G1 code, with the same refusals
 *   and texts (out_err256: nullable, 256 bytes).  gh_affine96 (nullable): the n = ell + 4 records vec_G | vec_H, for out_m48;
 *   out_m_scalars32: the n scalars of M's row, perm | vec_m_blinders. */
size_t cg1_whisk_shuffle_proof_bytes(size_t ell);                   /* 0 when cg1_shuffle_prover_proof_bytes(ell) is */
int cg1_whisk_shuffle_front(cg1_ctx* ctx, cg1_fixed* tab, size_t ell, size_t n_provers, const uint32_t* g_index, const uint32_t* h_index, const uint8_t* trackers96,
                            const uint32_t* perm, const uint8_t* k32, const uint8_t* vec_m_blinders32, uint8_t* out_rs_affine96, uint8_t* out_tu_affine96,
                            uint8_t* out_post96, uint8_t* out_m48);
int cg1_whisk_shuffle_prove_device(cg1_ctx* ctx, cg1_fixed* tab, size_t ell, size_t n_provers, const uint32_t* g_index, const uint32_t* h_index, const uint32_t* u_index,
                                   const uint32_t* gt_index, const uint32_t* gu_index, const uint8_t* gth_affine96, const uint8_t* trackers96, const uint32_t* perm,
                                   const uint8_t* k32, const uint8_t* vec_m_blinders32, const uint8_t* vec_a_blinders32, const uint8_t* vec_c_blinders32,
                                   const uint8_t* ipa_r32, const uint8_t* ipa_z_head32, const uint8_t* blinders32, const uint8_t* vec_r32, uint8_t* out_post96,
                                   uint8_t* out_proofs);
int cg1_whisk_shuffle_front_emulate(size_t ell, const uint8_t* trackers96, const uint32_t* perm, const uint8_t* k32, const uint8_t* vec_m_blinders32,
                                    const uint8_t* gh_affine96 /* nullable */, uint8_t* out_rs_affine96, uint8_t* out_tu_affine96, uint8_t* out_post96,
                                    uint8_t* out_m_scalars32, uint8_t* out_m48 /* with gh_affine96 */, char* out_err256 /* nullable */);

/* ---- Whisk shuffles proved from a SEED: the permutation, k and all 3 n + 14 blinders of every shuffle (n = ell + 4) are drawn on the
 * device.  For shuffle number index (global: first_index + position in the call, below 2^32) and draw number d,
 *   block(index, d) = SHAKE256("whisk_shuffle_draw" || seed32 || le64(index) || le32(d)).digest(64)      (62 bytes in: one permutation)
 *   d = 0 .. ell - 2        Fisher-Yates on perm = 0 .. ell - 1, in order of d: i = ell - 1 - d, j = le128(block[:16]) mod (i + 1), swap perm[i], perm[j]
 *   then, one draw each     k, vec_m_blinders (4), vec_a_blinders (2), vec_c_blinders (4), ipa_r (n), ipa_z_head (n - 2), r_t r_u r_a r_b r_k,
 *                           vec_r (n): le512(block) mod r.  A zero is not special-cased: the chain refuses what it refuses.
 * so a shuffle's output depends on (seed, index) alone, not on its neighbours or on how a batch is cut into calls.  A seed that is reused,
 * or known to anyone but the prover, reveals every k and permutation it proved.
 * cg1_whisk_shuffle_draws_device   k_whisk_draws + k_whisk_fisher_yates (csrc/kernels_whisk_shuffle.h) alone.  out_perm: n_provers x ell;
 *   out_scalars32: (3 n + 14) n_provers scalars in the COLUMN layout cg1_whisk_shuffle_prove_device takes -- k | vec_m_blinders |
 *   vec_a_blinders | vec_c_blinders | ipa_r | ipa_z_head | r_t .. r_k | vec_r, every column its n_provers rows one after the other.
 *   CG1_ERR_ARG, nothing written: a null pointer, ell + 4 not a power of two in 8 .. CG1_SAME_MSM_MAX_N, n_provers above
 *   CG1_WHISK_SHUFFLE_DRAWS_MAX_PROVERS, first_index + n_provers > 2^32.  The device buffer of the draws is zeroed before the call returns.
 * cg1_whisk_shuffle_draws          the host twin over the host Keccak: same format, same refusals (without a text: it has no context).
 * cg1_whisk_shuffle_prove_seeded   (1) those draws on the context's stream and one copy of them down; (2) cg1_whisk_shuffle_front with a
 *   status PER PROVER: out_status[p] = 0, CG1_WHISK_SHUFFLE_NO_DECODE or CG1_WHISK_SHUFFLE_NOT_G1, out_bad_at[p] = tracker 2 + half (0 = r_G,
 *   1 = k_r_G) of the prover's first such point -- points the decoder refuses before points outside G1, each in tracker order; (3) the
 *   provers with status 0 through cg1_shuffle_prove_device (all refused: CG1_OK without it).  A refused prover gets zero bytes in
 *   out_post96 and out_proofs and leaves the others as they would be without it.  Every other refusal is the whole call's, as
 *   cg1_whisk_shuffle_prove_device makes it, and leaves all four outputs untouched; a text of the chain counts the provers that reached it.
 *   Before returning, the device buffer of the draws and the table's staging block (both copies) are zeroed and the host staging of the
 *   draws is wiped; neither the seed nor a draw appears in an error text.
 *   With the context parameter "whisk_resident_witness" = 1 step (1) makes NO copy down: the draws stay in the context's draws buffer and
 *   k_whisk_witness_place (csrc/kernels_whisk_shuffle.h) copies them, on the device, into the witness fields of the front's and the chain's
 *   staging blocks, behind the uploads of the public fields and in front of the first kernel that reads them -- destination prover q from
 *   the q-th prover with status 0.  The host block's witness fields are never written, no gathered copy or staging vector is made, and the
 *   host checks on witness VALUES (scalars below r, permutation entries below ell, vec_c_blinders[2] != 0) are skipped: the draws are
 *   reduced mod r and permutations by construction, and the zero events set the chains' status bits on the device all the same.  The same
 *   bytes come out for the same seed.  The draws buffer is zeroed by a scope guard on every way out of the call.  What then still touches
 *   host memory of a call's secrets: the 32-byte seed (the caller's buffer, the kernel arguments).  cg1_chain_prove_seeded,
 *   cg1_whisk_shuffle_prove_device and cg1_whisk_shuffle_draws_device do not read the parameter.
 * cg1_whisk_last_witness_traffic   test support: of the last cg1_whisk_shuffle_prove_seeded call on the context, out[0] = witness bytes copied
 *   device -> host, out[1] = witness bytes the library wrote into host memory (staging, gathered rows, the blocks' witness fields).  Plain
 *   host counters, zeroed when a seeded call begins.  Both non-zero after a call that proved something on the copying path; 0 and 0 on the
 *   resident one.
 * cg1_whisk_draws_buffer_is_zero   test support: 1 when every byte of the context's draws buffer is zero (or it has none), 0 when not, -1
 *   on a HIP error.  One D2H copy.
 * cg1_whisk_witness_block_emulate  host only, no HIP call, test support: the front's (which_block = 0) or the chain's (1) staging block laid
 *   out as the seeded entry lays it out for P drawn shuffles, of which keep[0] < .. < keep[Q - 1] reach the chain (NULL: all; the front
 *   takes all P whatever keep says), with ONLY the witness fields filled from draws_block (swaps | perm | scalars as the draws buffer holds
 *   them, 64-byte aligned parts) -- resident = 0: by the copying path's gather and stage functions; resident = 1: by the placement map the
 *   kernel shares.  -> the block's length in bytes (0: a shape the entry refuses, a bad keep list, a null pointer).  out (cap bytes) is
 *   written only if cap >= that length; out_fields gets (offset, length) per witness field, up to the *n_fields pairs it holds on entry,
 *   and *n_fields becomes the number of fields. */
#define CG1_WHISK_SHUFFLE_DRAWS_MAX_PROVERS 4096
#define CG1_WHISK_SHUFFLE_NO_DECODE 2   /* a tracker point is not a compressed encoding of a curve point */
#define CG1_WHISK_SHUFFLE_NOT_G1    3   /* a tracker point lies outside the prime-order subgroup */
int cg1_whisk_shuffle_draws_device(cg1_ctx* ctx, size_t ell, size_t n_provers, const uint8_t* seed32, uint64_t first_index, uint32_t* out_perm, uint8_t* out_scalars32);
int cg1_whisk_shuffle_draws(size_t ell, size_t n_provers, const uint8_t* seed32, uint64_t first_index, uint32_t* out_perm, uint8_t* out_scalars32);
int cg1_whisk_shuffle_prove_seeded(cg1_ctx* ctx, cg1_fixed* tab, size_t ell, size_t n_provers, const uint32_t* g_index, const uint32_t* h_index, const uint32_t* u_index,
                                   const uint32_t* gt_index, const uint32_t* gu_index, const uint8_t* gth_affine96, const uint8_t* trackers96, const uint8_t* seed32,
                                   uint64_t first_index, uint8_t* out_post96, uint8_t* out_proofs, int32_t* out_status /* n_provers */, uint32_t* out_bad_at /* n_provers */);
void cg1_whisk_last_witness_traffic(const cg1_ctx* ctx, uint64_t out[2]);
int cg1_whisk_draws_buffer_is_zero(cg1_ctx* ctx);
size_t cg1_whisk_witness_block_emulate(size_t ell, size_t P, const size_t* keep, size_t Q, const uint8_t* draws_block, int resident, int which_block, uint8_t* out, size_t cap,
                                       uint64_t* out_fields, size_t* n_fields);

/* ---- A chain of Whisk shuffles PROVED over the resident tracker set (the set: cg1_chain_expand above; shuffle_chain.py).  Block j, in order,
 * reads pre_j = [set[i] for i in indices_j] before any of its own writes and, unless refused, writes set[indices_j[t]] = k_j * pre_j[perm_j[t]],
 * t = 0 .. ell - 1 in order (a repeated index: the last write wins).  A block is refused -- it writes nothing, its outputs are zeros, later
 * blocks read what was there -- when a pre point does not decode (CG1_WHISK_SHUFFLE_NO_DECODE) or lies outside G1 (CG1_WHISK_SHUFFLE_NOT_G1);
 * out_bad_at is tracker 2 + half of the first such point in cg1_whisk_shuffle_prove_seeded's order.
 * cg1_chain_lineage (host, no point arithmetic): point_status = 2 n_slots bytes (r_G of slot s at 2 s, k_r_G at 2 s + 1; 0, _NO_DECODE or
 *   _NOT_G1; only slots read at first touch are looked at).  The current value of a slot is composite * (the tracker its ORIGIN slot held
 *   before the call).  out_origin: [n_blocks][2][ell] origin slots, pre position t at [b][0][t], post position t at [b][1][t] (0xffffffff in
 *   a refused block); out_scalar32: the composites (products of the k's, mod r) in the same layout, canonical (zeros in a refused block);
 *   out_writers / out_n_writers as cg1_chain_expand's.  Every output may be NULL.  Refused before anything is written: CG1_ERR_ARG for
 *   ell = 0, an index >= n_slots, a perm row that is no permutation of 0 .. ell - 1, another point_status value; CG1_ERR_ENCODING for k >= r.
 * cg1_chain_evolve_device: the tracker stage on the context's stream -- the distinct slots read are certified (k_subgroup_row over their
 *   records, the first wait), the lineage, ONE k_chain_lineage_mul launch (csrc/kernels_chain_prove.h) for every pre and post point, the last
 *   writers' records scattered into the set with zero status bytes, the second wait.  out_post96: n_blocks x ell x (T48 | U48).
 *   out_stats (NULL or 2 floats): the stage's milliseconds between two events, the number of slots certified.  cg1_chain_lineage's refusals,
 *   with a text, before anything runs.  The composites' device field is zeroed and their host staging wiped before it returns.
 * cg1_chain_prove_seeded: block j's draws are those of shuffle first_index + j of cg1_whisk_shuffle_prove_seeded, and its post bytes, M || proof
 *   and status are what that entry gives for pre_j: the draws of all blocks (kept in wiped host staging), the tracker stage, then the surviving
 *   blocks through cg1_shuffle_prove_device in groups of CG1_SAME_MSM_MAX_PROVERS.  g_index (ell), h_index (4), u / gt / gu_index: the CRS in the
 *   table, once.  n_blocks <= CG1_WHISK_SHUFFLE_DRAWS_MAX_PROVERS.  out_stats (NULL or 4 floats): also the wall milliseconds inside
 *   cg1_shuffle_prove_device and of the whole call.  Secret hygiene as cg1_whisk_shuffle_prove_seeded's.
 * Neither device entry restores the set's records when it fails after the scatter: the caller, who holds the bytes, decodes them afresh. */
int cg1_chain_lineage(size_t n_slots, const uint8_t* point_status, const uint32_t* indices, const uint32_t* perm, const uint8_t* k32, size_t n_blocks, size_t ell,
                      int32_t* out_status, uint32_t* out_bad_at, uint32_t* out_origin, uint8_t* out_scalar32, uint32_t* out_writers, size_t* out_n_writers);
int cg1_chain_evolve_device(cg1_ctx* ctx, void* d_set_pts96, void* d_set_pstat, size_t n_slots, const uint32_t* indices, const uint32_t* perm, const uint8_t* k32,
                            size_t n_blocks, size_t ell, uint8_t* out_post96, int32_t* out_status, uint32_t* out_bad_at, uint32_t* out_writers, size_t* out_n_writers,
                            float* out_stats);
int cg1_chain_prove_seeded(cg1_ctx* ctx, cg1_fixed* tab, size_t ell, size_t n_blocks, const uint32_t* g_index, const uint32_t* h_index, uint32_t u_index, uint32_t gt_index,
                           uint32_t gu_index, const uint8_t* gth_affine96, void* d_set_pts96, void* d_set_pstat, size_t n_slots, const uint32_t* indices,
                           const uint8_t* seed32, uint64_t first_index, uint8_t* out_post96, uint8_t* out_proofs, int32_t* out_status, uint32_t* out_bad_at,
                           uint32_t* out_writers, size_t* out_n_writers, float* out_stats);

/* The tracker scan: which trackers does a set of Whisk secrets open?  For n_trackers trackers (r_G48 | k_r_G48, cg1_opening_prove's layout)
 * and n_ks secrets (scalar32), bit (i, j) = [ k_j * point_projective_from_bytes(r_G_i) == point_projective_from_bytes(k_r_G_i) ]
 * (util.py:35-36: unchecked decoding, a point outside G1 is legal and multiplied exactly; the relation opening.py proves).
 *   out_bitmap           n_trackers x ceil(n_ks / 64) 64-bit words, word (i, j / 64), bit j % 64; padding bits are zero
 *   out_tracker_status   per tracker: 0, or CG1_SHUFFLE_BAD_POINT when r_G or k_r_G does not decode (its row is zero)
 *   out_k_status         per secret: 0, or CG1_SHUFFLE_BAD_SCALAR when k >= r (its column is zero); k = 0 is a legal scalar
 *   tile_bases           trackers whose light tables (csrc/kernels_light.h: 128 KiB each) are resident at a time on the device; 0 = the
 *                        default CG1_TRACKER_MATCH_DEFAULT_TILE (128 MiB of records).  The host twin ignores the value but refuses the same ones.
 * Host buffers in and out; the device call runs on the context's stream and waits once.  Refusals come before anything is written:
 * CG1_ERR_ARG for a null buffer, n_trackers > CG1_TRACKER_MATCH_MAX_TRACKERS, n_ks > CG1_TRACKER_MATCH_MAX_KS, a bitmap above
 * CG1_TRACKER_MATCH_MAX_BITMAP_BYTES or tile_bases > CG1_TRACKER_MATCH_MAX_TILE (larger jobs: call in chunks of trackers and secrets, as
 * the Python face does).  No error text ever holds a secret, and the device copy of the secrets is zeroed and freed before the call returns.
 * cg1_tracker_match is the host twin on the worker pool (decode, multiply, compare): the same bits and statuses, what a machine without
 * a GPU and small calls take.  cg1_tracker_match_last_ms: with the context parameter "tracker_scan_timing" = 1 the device call waits
 * between its phases and keeps the wall milliseconds of the table builds (ms[0]) and the match kernels (ms[1]) of the last call.
 * Up to CG1_TRACKER_MATCH_LADDER_MAX_KS secrets (context parameter "tracker_scan_ladder_max_ks", 0 .. 1024; 0 = never) the device call
 * builds no table: it runs one double-and-add ladder per pair (k_batch_mul) and compares the affine results on the device -- the same
 * bits and statuses, cheaper below the measured crossover; ms[0] is then 0. */
#define CG1_TRACKER_MATCH_MAX_TRACKERS     65536
#define CG1_TRACKER_MATCH_MAX_KS           1048576
#define CG1_TRACKER_MATCH_MAX_BITMAP_BYTES (1ull << 30)
#define CG1_TRACKER_MATCH_MAX_TILE         4096
#define CG1_TRACKER_MATCH_DEFAULT_TILE     1024
#define CG1_TRACKER_MATCH_LADDER_MAX_KS    32   /* up to this many secrets the device call runs one ladder per pair instead of the tables */
int cg1_tracker_match_device(cg1_ctx* ctx, const uint8_t* trackers96 /* r_G | k_r_G */, size_t n_trackers, const uint8_t* ks32, size_t n_ks,
                             size_t tile_bases, uint64_t* out_bitmap, int32_t* out_tracker_status, int32_t* out_k_status);
int cg1_tracker_match(const uint8_t* trackers96 /* r_G | k_r_G */, size_t n_trackers, const uint8_t* ks32, size_t n_ks, size_t tile_bases,
                      uint64_t* out_bitmap, int32_t* out_tracker_status, int32_t* out_k_status);
int cg1_tracker_match_last_ms(const cg1_ctx* ctx, float ms[2]);

/* Whisk REGISTRATIONS made in bulk: per secret k the tracker (r_G48 | k_r_G48, generate_tracker, test_curdleproofs.py:759-790), the
 * k_commitment k_G48 (get_k_commitment) and the opening proof A48 | B48 | s32 (GenerateWhiskTrackerProof, whisk_interface.py:177-190).
 * The maker knows r, so all five points are multiples of the generator and come from the context's table of G with ONE inversion per
 * item (csrc/kernels_register.h), with no square root and no doubling ladder:
 *     r_G = r G    k_r_G = (k r mod r_order) G    k_G = k G    A = b G    B = (b r mod r_order) G
 * then the "whisk_opening_proof" transcript over [k_G, G, k_r_G, r_G, A, B], the challenge c and s = b - c k (opening.py:42-56).
 * With (r, b) supplied the bytes ARE the reference's when it draws that r and that b.  Item i of a call has the global index
 * first_index + i < 2^32; its output depends on (k, r, b) -- or (k, seed, index) -- alone, not on its neighbours or on how a batch is cut.
 *   rs32, blinders32   both given (n x scalar32 each) or both NULL.  NULL: r and b of an item are derived from seed32,
 *                        block(index, d) = SHAKE256("whisk_registration_draw" || seed32 || le64(index) || le32(d)).digest(64)
 *                        r = int.from_bytes(block(index, 0), "little") mod r_order,  b likewise with d = 1
 *                      (cg1_whisk_register_draws is the host's copy).  A seed that is reused or known to anyone else reveals every k it
 *                      was used with (k = (b - s) / c): 32 fresh bytes from the OS per call, a fixed one only in tests.
 *   status[i]          0 made; CG1_SHUFFLE_BAD_SCALAR: k >= r_order; CG1_OPENING_BAD_BLINDER: an r or b, supplied or derived, that is zero
 *                      or >= r_order.  k = 0 is legal (k_r_G and k_G are then the identity, 0xC0 00 .. 00).  A refused item gets zero
 *                      bytes in all three outputs and leaves its neighbours alone.
 * Host buffers in and out.  CG1_ERR_ARG, before anything is written, for n >= CG1_WHISK_REGISTER_MAX_ITEMS, first_index + n > 2^32, a null
 * buffer, or only one of rs32 / blinders32.  The device call runs slices of 2^20 items on the context's stream and zeroes the device
 * copies of k, r, b, k r and b r before it returns; no error text ever holds a secret.  cg1_whisk_register is the host twin on the
 * worker pool (the same bytes and codes; it takes supplied r and b only).
 * cg1_whisk_register_points_device is the stage of the five multiples alone, for measurements: five columns of n <= 2^20 canonical
 * scalars -> five columns of n encodings (device pointers); shared_inversion != 0 runs k_register_points (one lane and one inversion per
 * item: what the device call uses for slices above 32 768 items), 0 runs k_generator_mul over the 5 n scalars (one lane and one inversion
 * per point: what it uses up to there, where the longer lanes of the first leave the chip idle). */
#define CG1_WHISK_REGISTER_MAX_ITEMS (1ull << 26)
int cg1_whisk_register_device(cg1_ctx* ctx, size_t n, const uint8_t* ks32, const uint8_t* rs32 /* or NULL */, const uint8_t* blinders32 /* or NULL */,
                              const uint8_t* seed32 /* used when rs32 == NULL */, uint64_t first_index, uint8_t* out_trackers96, uint8_t* out_k_commitments48,
                              uint8_t* out_proofs128, int32_t* status);
int cg1_whisk_register(size_t n, const uint8_t* ks32, const uint8_t* rs32, const uint8_t* blinders32, uint8_t* out_trackers96, uint8_t* out_k_commitments48,
                       uint8_t* out_proofs128, int32_t* status);
int cg1_whisk_register_draws(const uint8_t seed32[32], uint64_t first_index, size_t n, uint8_t* out_rs32, uint8_t* out_blinders32);
int cg1_whisk_register_points_device(cg1_ctx* ctx, const void* d_scalars32, size_t n, void* d_out48, int shared_inversion);

#ifdef __cplusplus
}
#endif
#endif /* CURDLE_G1_H */
