"""Whisk opening-proof GENERATION on one GPU (curdleproofs_pie_amd.opening_prover): one JSON line with
  - proofs/s of the packed path with seed-derived blinders at n = 1, 4, 64, 1 024, 65 536 (device; the host twin beside it up to 64);
  - per-stage times at n = 65 536 through cg1_timer_begin / cg1_timer_end (decompression, the fixed-base kernel, B = b r_G, compression;
    the transcripts and the rest as the remainder of the whole call);
  - generator multiples: cg1_generator_mul_device against cg1_batch_mul_device(nbase = 1) at 2^20 in the same run, and the fixed-base
    kernel's estimated multiply-adds per second against the chip's v_mad_u64_u32 rate (cg1_probe_mad_rate);
  - the n = 1 latency of generate_whisk_tracker_proof against the reference's GenerateWhiskTrackerProof control flow
    (whisk_interface.py:177-190 -> opening.py:33-56) run over the product's G1Point / Scalar / transcript face, same bytes required.
Best of --reps after a warm-up call each.

    python tools/gpu_opening_prover_timing.py [--reps 5] [--package-root DIR] [--gen-only]
"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# estimated v_mad_u64_u32 per fixed-base output (c = 8): ~all 32 windows carry a digit, a mixed addition is 8 M + 2 S, one inversion
# (fp_pow6: ~378 S + ~109 M) and 6 products around it; ~323 multiply-adds per field product (148 862 for the 461 of a square root)
MADS_PER_PRODUCT = 323
FIXED_BASE_PRODUCTS = 32 * 10 + 487 + 6


def best(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return min(out)


def best_timer(ctx, fn, reps):
    fn()
    out = []
    for _ in range(reps):
        ctx.timer_begin()
        fn()
        out.append(ctx.timer_end())
    return min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--package-root", default=ROOT, help="tree to import curdleproofs_pie_amd from (A/B of a variant build)")
    ap.add_argument("--gen-only", action="store_true", help="only the generator-multiples comparison")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.abspath(a.package_root))
    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd import opening_prover as P

    ctx = N.Context(0)
    rec = {"tool": "gpu_opening_prover_timing", "package_root": os.path.relpath(os.path.abspath(a.package_root), ROOT), "reps": a.reps}
    # ---- generator multiples at 2^20
    n = 1 << 20
    d_sc, d_out = ctx.alloc(32 * n), ctx.alloc(96 * n)
    d_g = ctx.alloc(96)
    g = ctypes.create_string_buffer(N.POINT_BYTES)
    N.cg1_generator(g)
    g96 = ctypes.create_string_buffer(96)
    N.cg1_to_affine96(g96, g.raw)
    d_g.upload(g96.raw)
    ctx.check(N.cg1_gen_scalars_device(ctx.handle, d_sc.ptr, n, 99))
    t_fixed = best_timer(ctx, lambda: ctx.check(N.cg1_generator_mul_device(ctx.handle, d_sc.ptr, n, d_out.ptr, None)), a.reps)
    fixed = d_out.download(96 * 4096)
    t_mul = best_timer(ctx, lambda: ctx.check(N.cg1_batch_mul_device(ctx.handle, d_g.ptr, 1, d_sc.ptr, d_out.ptr, n)), a.reps)
    assert d_out.download(96 * 4096) == fixed, "fixed-base outputs differ from k_batch_mul's"
    mad_rate = ctx.probe_mad_rate()
    rec["generator_2p20"] = {"fixed_base_ms": round(t_fixed, 3), "batch_mul_nbase1_ms": round(t_mul, 3), "speedup": round(t_mul / t_fixed, 2),
                             "fixed_base_outputs_per_s": round(n / t_fixed * 1e3), "est_mads_per_output": FIXED_BASE_PRODUCTS * MADS_PER_PRODUCT,
                             "mad_rate_lane_ops_per_s": mad_rate,
                             "fraction_of_mad_rate": round(n * FIXED_BASE_PRODUCTS * MADS_PER_PRODUCT / (t_fixed * 1e-3) / mad_rate, 3)}
    for b in (d_sc, d_out, d_g):
        b.free()
    if a.gen_only:
        print(json.dumps(rec))
        return
    # ---- the packed prover, seed-derived blinders
    rng = random.Random(1)
    base_n = 1024
    from curdleproofs_pie_amd.shuffle_verifier import FR_MODULUS as R

    rs32 = b"".join(rng.randint(1, R - 1).to_bytes(32, "little") for _ in range(base_n))
    ks32 = b"".join(rng.randint(1, R - 1).to_bytes(32, "little") for _ in range(base_n))
    rG = ctypes.create_string_buffer(96 * base_n)
    krG = ctypes.create_string_buffer(96 * base_n)
    assert N.cg1_batch_mul_add_pool(g96.raw, 1, rs32, base_n, None, rG, base_n, 0) == 0
    assert N.cg1_batch_mul_add_pool(rG.raw, base_n, ks32, base_n, None, krG, base_n, 0) == 0
    c48 = ctypes.create_string_buffer(48)
    tr = []
    for i in range(base_n):
        for src in (rG, krG):
            blob = ctypes.create_string_buffer(N.POINT_BYTES)
            N.cg1_from_affine96(blob, src.raw[96 * i: 96 * i + 96], 0)
            N.cg1_compress(c48, blob.raw)
            tr.append(c48.raw)
    trk1024 = b"".join(tr)
    seed = hashlib.sha256(b"timing").digest()
    dev, host = P.OpeningBatchProver(ctx, device=True), P.OpeningBatchProver(ctx, device=False)
    rows = {}
    for m in (1, 4, 64, 1024, 65536):
        reps_m = (m + base_n - 1) // base_n
        t_, k_ = (trk1024 * reps_m)[: 96 * m], (ks32 * reps_m)[: 32 * m]
        td = best(lambda: dev.prove_packed(t_, k_, seed=seed), a.reps)
        row = {"device_ms": round(td * 1e3, 3), "device_proofs_per_s": round(m / td)}
        assert dev.last_status == [0] * m
        if m <= 64:
            th = best(lambda: host.prove_packed(t_, k_, seed=seed), a.reps)
            row.update(host_ms=round(th * 1e3, 3), host_proofs_per_s=round(m / th))
            assert host.prove_packed(t_, k_, seed=seed) == dev.prove_packed(t_, k_, seed=seed)
        rows[str(m)] = row
    rec["prove_packed"] = rows
    # ---- stages at n = 65 536 (each alone on the device, device buffers)
    m = 65536
    t_, k_ = (trk1024 * 64), (ks32 * 64)
    d_t, d_aff, d_st = ctx.alloc(96 * m), ctx.alloc(192 * m), ctx.alloc(2 * m)
    d_k, d_g48, d_b = ctx.alloc(64 * m), ctx.alloc(96 * m), ctx.alloc(96 * m)
    d_t.upload(t_)
    d_k.upload(k_ + k_)
    stages = {"whole_call_ms": rows["65536"]["device_ms"]}
    stages["decompress_2n_ms"] = best_timer(ctx, lambda: ctx.check(N.cg1_batch_decompress_device(ctx.handle, d_t.ptr, d_aff.ptr, d_st.ptr, 2 * m, 0)), a.reps)
    stages["generator_2n_ms"] = best_timer(ctx, lambda: ctx.check(N.cg1_generator_mul_device(ctx.handle, d_k.ptr, 2 * m, None, d_g48.ptr)), a.reps)
    stages["b_times_rG_n_ms"] = best_timer(ctx, lambda: ctx.check(N.cg1_batch_mul_add_device(ctx.handle, d_aff.ptr, m, d_k.ptr, m, None, d_b.ptr, m)), a.reps)
    stages["compress_n_ms"] = best_timer(ctx, lambda: ctx.check(N.cg1_batch_compress_device(ctx.handle, d_b.ptr, d_g48.ptr, m)), a.reps)
    stages = {k: round(v, 3) for k, v in stages.items()}
    stages["transcripts_and_rest_ms"] = round(stages["whole_call_ms"] - sum(v for k, v in stages.items() if k != "whole_call_ms"), 3)
    rec["stages_65536"] = stages
    for b in (d_t, d_aff, d_st, d_k, d_g48, d_b):
        b.free()
    # ---- n = 1: the drop-in against the reference's control flow over the product's face
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript

    G1 = G1Point()

    def reference_flow(tracker, k):                          # whisk_interface.py:177-190, opening.py:33-56
        transcript = CurdleproofsTranscript(b"whisk_opening_proof")
        k_r_G = G1Point.from_compressed_bytes_unchecked(tracker[1])
        r_G = G1Point.from_compressed_bytes_unchecked(tracker[0])
        k_G = G1 * k
        blinder = Scalar.from_le_bytes(random.randint(1, R - 1).to_bytes(32, "little"))
        A = G1 * blinder
        B = r_G * blinder
        for p in (k_G, G1, k_r_G, r_G, A, B):
            transcript.append_message(b"tracker_opening_proof", bytes(p.to_compressed_bytes()))
        c = transcript.get_and_append_challenge(b"tracker_opening_proof_challenge")
        s = blinder - c * k
        return bytes(A.to_compressed_bytes()) + bytes(B.to_compressed_bytes()) + bytes(s.to_le_bytes())

    tracker = (trk1024[:48], trk1024[48:96])
    k1 = Scalar.from_le_bytes(ks32[:32])
    random.seed(5)
    want = reference_flow(tracker, k1)
    random.seed(5)
    assert P.generate_whisk_tracker_proof(tracker, k1, ctx) == want, "drop-in differs from the reference control flow"
    rec["n1_latency_ms"] = {"generate_whisk_tracker_proof": round(best(lambda: P.generate_whisk_tracker_proof(tracker, k1, ctx), a.reps) * 1e3, 3),
                            "reference_flow_over_product_face": round(best(lambda: reference_flow(tracker, k1), a.reps) * 1e3, 3)}
    rec["floors"] = {"generator_ge_3x": rec["generator_2p20"]["speedup"] >= 3.0, "prover_ge_1e6_per_s_at_65536": rows["65536"]["device_proofs_per_s"] >= 1e6}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
