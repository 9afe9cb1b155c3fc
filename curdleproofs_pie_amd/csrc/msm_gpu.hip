// MI355X (gfx950) Pippenger MSM over BLS12-381 G1 -- the per-device pipeline context, the launch chains of the
// two regimes and the C ABI.  The kernels live in kernels_*.h (one translation unit, included below).
//
// Replaces the hot loop of the reference's compute_MSM
//   (/root/reference/curdleproofs/curdleproofs/msm_accumulator.py:6-12:  current += base * scalar)
// with a signed-digit windowed-bucket method laid out for CDNA4.  Regime A (one large MSM), in launch order:
//
//   k_prepare_points   96 B affine (std form) -> 128 B records (x,y as 14x28-bit Montgomery limbs): one aligned
//                      cache line per point, so the bucket gather touches exactly one line     [kernels_prepare_digits.h]
//   k_digits           c-bit signed digits of this rank's windows, window-major u16
//   k_part_count/scatter + k_uscan*, k_bin_sort
//                      two-level LDS partition sort by (window, bucket); no global atomics     [kernels_sort.h]
//                      (k_hist/k_scatter: global-atomic counting sort, only for n > 2^23)
//   k_scan1/2/3, k_chunk_desc, k_len_scan, k_order
//                      bucket offsets; chunks of <= L entries, <= 4096 chunks per bucket (L: "chunk_len", 8, doubled while
//                      entries / 2^18 exceeds it; without shards at least 10 from 2^20 entries and, from 2^21 to 2^24 entries
//                      over more than 2^18 buckets, a whole bucket -- mean load + 8 sigma + 1, below 2^22 entries 20 at most);
//                      chunks ordered by descending length so a wave's lanes finish together
//   k_accumulate  ***  the dominant kernel: one lane per chunk, XYZZ mixed adds over gathered points [kernels_accumulate.h]
//   k_heavy_combine, k_bucket_fold
//                      re-join buckets that were cut into several chunks (skewed scalars, window-sharded ranks)
//   k_rowcol, k_small_tree
//                      2-D bucket reduction: row sums / column sums, then 1 + hb + lb masked sums per window,
//                      exported as canonical XYZZ words                                        [kernels_reduce.h]
//   host tail          one Horner over global bit positions (255 doublings + 256 additions, host_g1.cpp): one GPU
//                      lane needs ~20-30 us per dependent EC operation, a host core ~0.5 us, so the strictly serial
//                      tail belongs on the host.
// Regime B (cg1_msm_batched*): k_group_count/scatter (LDS counting sort per (msm, window)), the same chunking +
// k_accumulate, k_seg_reduce, k_group_reduce, k_msm_horner.
//
// No MFMA: this is carry-propagating big-integer arithmetic.  The bound is the VALU integer-multiply rate
// (v_mad_u64_u32), see fp28.h; bench.py reports both that and the HBM roofline the task sheet asks for.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <string>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include "g1_xyzz.h"
#include "g1_quad.h"
#include "host_g1.h"
#include "lazy_host.h"
#include "pool.h"
#include "secret_wipe.h"
#include "../../include/curdle_g1.h"

namespace cg1 {

int pick_window(size_t n);

#include "kernels_records.h"
#include "fp_row.h"
#include "glv.h"
#include "kernels_prepare_digits.h"
#include "kernels_sort.h"
#include "kernels_accumulate.h"
#include "kernels_reduce.h"
#include "kernels_small.h"
#include "kernels_batch.h"
#include "kernels_generator.h"
#include "fixed_digits.h"
#include "kernels_fixed.h"
#include "light_digits.h"
#include "kernels_light.h"
#include "kernels_tracker_scan.h"
#include "kernels_exact.h"         // k_exact_relations: signed sums of at most four k P == identity, exact on all of E(Fp), a wave per relation
#include "kernels_tracker_set.h"   // k_chain_gather / k_chain_scatter: decoded records between a batch's points and the resident tracker set
}  // namespace cg1
#include "kernels_rows.h"
#include "kernels_merlin.h"
#include "kernels_frontend.h"
#include "kernels_opening.h"
#include "kernels_register.h"      // k_register_scalars / k_register_points: Whisk registrations, five multiples of G per lane with one inversion
#include "kernels_chain.h"         // the step skeleton of the device provers: lane-0 transcript, status merge, inversion, clocks
#include "kernels_ipa.h"           // k_ipa_step: the inner-product argument's phases, op tables and Fr steps over that skeleton
#include "kernels_same_msm.h"      // k_smsm_step: the same-MSM argument's
#include "kernels_gprod.h"         // k_gprod_step: the grand-product argument's, up to the hand-over to k_ipa_step
#include "kernels_same_perm.h"     // k_same_perm_begin: the same-permutation argument's head in front of k_gprod_step's step phase
#include "kernels_same_scalar.h"   // k_sscalar_step: the same-scalar block's two phases around its one MSM launch
#include "kernels_shuffle.h"       // k_shuffle_begin: the terms of a whole shuffle proof that depend on no later challenge than vec_a
#include "kernels_whisk_shuffle.h" // k_whisk_permute_mul: the post-shuffle trackers of a Whisk shuffle, k vec_R | k vec_S through the permutation
#include "kernels_chain_prove.h"   // k_chain_lineage_mul: every pre and post tracker of a proved chain from (origin slot, composite scalar), one launch
#include "host_context.h"          // Ctx: streams, helper threads, scratch buffers
#include "msm_plan.h"              // the pure call planner: who serves a call, every number its chain derives, the tail word
#include "host_chains.h"           // the launch chains as stages over a plan: regime A, k_msm_small, regime B
#include "capi_core_msm.h"         // cg1_* : host operators, context, memory, parameters, MSM entry points
#include "capi_vec_batched.h"      // resident vectors, batched normalisation, regime B
#include "capi_lincomb.h"          // deferred G1Point evaluation: cg1_lincomb_batch, cg1_batch_subgroup
#include "capi_timing_batchmul.h"  // timings / counters, cg1_batch_mul_add*
#include "capi_codec_transcripts.h"// decompression, subgroup flags, Merlin batches, opening proofs (verifier front-end, prover), k G
#include "capi_frontend.h"         // the shuffle verifier front-end on the device
#include "capi_rows_probes.h"      // scalar rows, compression, synthetic scalars, probes
#include "capi_fixed.h"            // resident fixed-base tables: cg1_fixed_*
#include "capi_chain.h"            // the host layer of a device prover's launch chain: layout, shared refusals, staging, tail
#include "capi_ipa.h"              // the inner-product argument proved on the device: cg1_ipa_prove_device
#include "capi_light.h"            // light tables of variable bases: cg1_light_*
#include "capi_same_msm.h"         // the same-MSM argument proved on the device: cg1_same_msm_prove_device
#include "capi_gprod.h"            // the grand-product argument proved on the device: cg1_gprod_prove_device
#include "capi_same_perm.h"        // the same-permutation argument proved on the device: cg1_same_perm_prove_device
#include "capi_same_scalar.h"      // the same-scalar block proved on the device: cg1_same_scalar_prove_device
#include "capi_shuffle.h"          // a whole shuffle proof proved on the device: cg1_shuffle_prove_device
#include "capi_whisk_shuffle.h"    // GenerateWhiskShuffleProof from tracker bytes: cg1_whisk_shuffle_front, cg1_whisk_shuffle_prove_device
#include "capi_exact.h"           // exact relations in bulk: cg1_exact_relations_device (host twin: csrc/shuffle_verify.cpp)
#include "capi_tracker_set.h"     // a chain of shuffles over a resident tracker set: strided decoding, cg1_chain_gather_enqueue / _scatter_enqueue
#include "capi_chain_prove.h"     // a chain of shuffles PROVED over the resident set: cg1_chain_evolve_device, cg1_chain_prove_seeded (host lineage: chain_lineage.h)
#include "capi_tracker_scan.h"    // which trackers a set of secrets opens: cg1_tracker_match_device and its host twin cg1_tracker_match
#include "capi_register.h"        // Whisk registrations in bulk: cg1_whisk_register_device, its host twin cg1_whisk_register, cg1_whisk_register_draws
