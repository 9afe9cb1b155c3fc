#!/usr/bin/env python3
"""A chain of Whisk shuffles verified over a device-resident tracker set (shuffle_chain.ShuffleChainVerifier) against the same blocks
expanded on the host and verified as self-contained items (ShuffleBatchVerifier.verify_stream).

Workload: ell = 124, a set of 16 384 trackers, --batches (>= 8) batches of 1 024 blocks; every block names 124 distinct pseudo-random slots.
The proofs are made on the device in rounds of 128 index-disjoint blocks per generate_packed call, each round over the set as the rounds
before it left it, so after the first batch nearly every pre tracker is an earlier block's post.

  chain       verify_blocks_packed over all batches in ONE call with SPLIT = 1 024 on the instance: internal batches of 1 024 blocks in
              flight on the one pipeline; the set is put back to its initial state (one decoding launch over 32 768 points) before every
              pass, outside the clock
  chain2048   the same call with the class's own SPLIT = 2 048: what verify_blocks_packed does with 8 192 blocks when nobody sets anything
  one         the expanded instances (expanded outside the clock) through verify_stream of a ShuffleBatchVerifier(pipelines=1, coalesce=0):
              the like-for-like comparison
  default     the same through the default ShuffleBatchVerifier: what a user would otherwise run
  kernels     hipEvents around single launches on an idle stream, median of 20: the plain decoding of 1 024 x L points, the strided decoding of
              1 024 x (L - 2 ell) and the gather of 1 024 x 2 ell records (not a trace of the pipeline: the kernels alone)

Every arm is a process of its own (a fresh HIP runtime each); `one` and `default` run from --baseline-tree when given -- a build of the
parent commit -- else from this tree.  The arms alternate for --rounds rounds; each process warms up with one pass over all batches and
times --passes passes (wall clock around calls that end in the statuses).  Blocks/s = blocks of a pass / median pass time.  Statuses are
checked (all 0) in every pass.

    python tools/gpu_chain_verify_timing.py [--batches 8] [--rounds 3] [--passes 3] [--baseline-tree DIR] > profiles/r20_chain_verify_timing.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELL, NB, SLOTS, BATCH, ROUND = 124, 4, 16384, 1024, 128


def make_workload(path, batches, seed):
    import ctypes
    import functools
    import random
    import types

    import numpy as np

    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point
    from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver

    rng = random.Random(seed)
    r = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    ctx = N.default_context()

    def multiples_of_g(count):
        """count x compressed48 of G * k for fresh k"""
        g, aff = ctypes.create_string_buffer(N.POINT_BYTES), ctypes.create_string_buffer(96)
        N.cg1_generator(g)
        N.cg1_to_affine96(aff, g.raw)
        sc = b"".join(rng.randint(1, r - 1).to_bytes(32, "little") for _ in range(count))
        raw = ctx.batch_mul_add_host(aff.raw, 1, sc, count, None, count)
        blobs, out = ctypes.create_string_buffer(N.POINT_BYTES * count), ctypes.create_string_buffer(48 * count)
        assert N.cg1_batch_from_affine96(blobs, raw, count) == 0
        N.cg1_batch_compress(out, blobs.raw, count)
        return out.raw

    n = ELL + NB
    enc = multiples_of_g(n + 3)
    pts = [G1Point.from_compressed_bytes_unchecked(enc[48 * i: 48 * i + 48]) for i in range(n + 3)]
    crs = types.SimpleNamespace(vec_G=pts[:ELL], vec_H=pts[ELL:n], H=pts[n], G_t=pts[n + 1], G_u=pts[n + 2])
    add = lambda v: functools.reduce(lambda a, b: a + b, v)
    crs_bytes = enc + bytes(add(crs.vec_G).to_compressed_bytes()) + bytes(add(crs.vec_H).to_compressed_bytes())
    table = FixedBaseTable(pts)
    prover = ShuffleBatchProver(crs, table=table)
    state = np.frombuffer(multiples_of_g(2 * SLOTS), dtype=np.uint8).reshape(SLOTS, 96).copy()
    initial = state.tobytes()
    nprng = np.random.default_rng(seed)
    idx_all, posts_all, proofs_all, inst_all = [], [], [], []
    t0 = time.perf_counter()
    for rnd in range(batches * BATCH // ROUND):
        idx = nprng.permutation(SLOTS)[: ROUND * ELL].astype("<u4").reshape(ROUND, ELL)      # index-disjoint blocks of distinct slots
        pre = state[idx]                                                                    # ROUND x ELL x 96
        post, proofs, status = prover.generate_packed(pre.tobytes(), seed=bytes([seed % 256]) * 32, first_index=rnd * ROUND)
        assert status == [0] * ROUND
        post = np.frombuffer(post, dtype=np.uint8).reshape(ROUND, ELL, 96)
        state[idx] = post
        inst = np.concatenate([pre[:, :, :48], pre[:, :, 48:], post[:, :, :48], post[:, :, 48:]], axis=1)      # vec_R | vec_S | vec_T | vec_U
        idx_all.append(idx); posts_all.append(post); proofs_all.append(np.frombuffer(proofs, dtype=np.uint8)); inst_all.append(inst)
    table.close()
    np.savez(path, crs=np.frombuffer(crs_bytes, dtype=np.uint8), initial=np.frombuffer(initial, dtype=np.uint8), idx=np.concatenate(idx_all),
             posts=np.concatenate(posts_all), proofs=np.concatenate(proofs_all), inst=np.concatenate(inst_all), final=state)
    print(json.dumps({"made": batches * BATCH, "prove_s": round(time.perf_counter() - t0, 2)}), flush=True)


def run_arm(arm, path, passes):
    import ctypes

    import numpy as np

    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd.shuffle_verifier import ShuffleBatchVerifier

    w = np.load(path)
    crs, n = w["crs"].tobytes(), len(w["idx"])
    res = {"arm": arm, "blocks": n, "hw_queues": N.hw_queues()}
    if arm == "kernels":
        ctx = N.Context(0)
        v = ShuffleBatchVerifier(crs, ctx)
        L = v.crs.points_per_proof
        wire = ctypes.create_string_buffer(BATCH * L * 48)
        assert N.cg1_shuffle_gather_points(v.crs.handle, BATCH, w["inst"][:BATCH].tobytes(), w["proofs"].tobytes()[: BATCH * v.crs.proof_bytes], wire) == 0
        d_w, d_p, d_s = ctx.alloc(BATCH * L * 48), ctx.alloc(BATCH * L * 96), ctx.alloc(BATCH * L)
        d_sp, d_ss = ctx.alloc(2 * SLOTS * 96), ctx.alloc(2 * SLOTS)
        d_w.upload(wire.raw)
        plan = (ctypes.c_int32 * (BATCH * 2 * ELL))(*[~(i % (2 * SLOTS)) for i in range(BATCH * 2 * ELL)])
        launches = {
            "decode_full_ms": lambda: N.cg1_batch_decompress_enqueue(ctx.handle, d_w.ptr, d_p.ptr, d_s.ptr, BATCH * L, 0),
            "decode_strided_ms": lambda: N.cg1_batch_decompress_strided_enqueue(ctx.handle, d_w.ptr, d_p.ptr, d_s.ptr, BATCH, L, 2 * ELL, L - 2 * ELL),
            "gather_ms": lambda: N.cg1_chain_gather_enqueue(ctx.handle, d_p.ptr, d_s.ptr, BATCH * L, d_sp.ptr, d_ss.ptr, 2 * SLOTS, plan, 0, BATCH, L, 2 * ELL),
        }
        ms = ctypes.c_float(0)
        for name, launch in launches.items():
            samples = []
            for rep in range(22):
                ctx.check(N.cg1_timer_begin(ctx.handle))
                ctx.check(launch())
                ctx.check(N.cg1_timer_end(ctx.handle, ctypes.byref(ms)))
                samples.append(ms.value)
            res[name] = round(statistics.median(samples[2:]), 4)
        res["points_full"], res["points_strided"] = BATCH * L, BATCH * (L - 2 * ELL)
        print(json.dumps(res), flush=True)
        return
    times = []
    if arm.startswith("chain"):
        from curdleproofs_pie_amd.shuffle_chain import ShuffleChainVerifier, TrackerSet

        ts = TrackerSet(w["initial"].tobytes(), N.Context(0))
        v = ShuffleChainVerifier(crs, ts)
        if arm == "chain":
            v.SPLIT = BATCH
        idx, posts, proofs = w["idx"].reshape(-1), w["posts"].tobytes(), w["proofs"].tobytes()
        for p in range(passes + 1):
            ts.replace(w["initial"].tobytes())
            t0 = time.perf_counter()
            st = v.verify_blocks_packed(idx, posts, proofs, n)
            times.append(time.perf_counter() - t0)
            assert st == [0] * n and ts.packed() == w["final"].tobytes()
        res.update(split=v.SPLIT, device_front_end=v.verifier.device_front_end, decoded_points=v.last_stats["decoded_points"], gathered_points=v.last_stats["gathered_points"],
                   decompress_stage_ms_per_batch=round(1e3 * v.last_stats["decompress_s"] / (n // BATCH), 3))
    else:
        v = ShuffleBatchVerifier(crs, N.Context(0), **({"pipelines": 1, "coalesce": 0} if arm == "one" else {}))
        pb = v.crs.proof_bytes
        proofs = w["proofs"].tobytes()
        batches = [(w["inst"][a: a + BATCH].tobytes(), proofs[a * pb: (a + BATCH) * pb], BATCH) for a in range(0, n, BATCH)]
        for p in range(passes + 1):
            t0 = time.perf_counter()
            st = [s for part in v.verify_stream(batches) for s in part]
            times.append(time.perf_counter() - t0)
            assert st == [0] * n
        res.update(device_front_end=v.device_front_end, pipelines=v.pipelines, coalesce=v.coalesce)
    res.update(pass_s=[round(t, 4) for t in times[1:]], blocks_per_s=round(n / statistics.median(times[1:])))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--baseline-tree")
    ap.add_argument("--arm", choices=("make", "chain", "chain2048", "one", "default", "kernels"))
    ap.add_argument("--workload")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.arm:
        sys.path.insert(0, a.tree)
        return make_workload(a.workload, a.batches, a.seed) if a.arm == "make" else run_arm(a.arm, a.workload, a.passes)
    assert a.batches >= 8, "steady state: at least eight batches"
    with tempfile.TemporaryDirectory(prefix="chain_timing_") as td:
        path = os.path.join(td, "workload.npz")

        def child(arm, tree):
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--workload", path, "--tree", tree, "--batches", str(a.batches), "--passes", str(a.passes),
                   "--seed", str(a.seed)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if done.returncode:
                sys.exit("arm %s failed (%d):\n%s" % (arm, done.returncode, done.stderr[-4000:]))
            return json.loads(done.stdout.strip().splitlines()[-1])

        print("# %d batches of %d blocks at ell = %d over %d slots; rounds of %d index-disjoint blocks; %s" % (
            a.batches, BATCH, ELL, SLOTS, ROUND, json.dumps(child("make", ROOT))), flush=True)
        base = a.baseline_tree or ROOT
        print("# baselines (one, default) run from %s" % ("a build of the parent commit" if a.baseline_tree else "this tree"), flush=True)
        runs = {"chain": [], "chain2048": [], "one": [], "default": []}
        for rnd in range(a.rounds):                          # the arms alternate
            for arm in runs:
                r = child(arm, ROOT if arm.startswith("chain") else base)
                runs[arm].append(r)
                print(json.dumps(r), flush=True)
        print(json.dumps(child("kernels", ROOT)), flush=True)
        print("# blocks/s, median of the rounds' medians (min .. max over rounds)")
        for arm, rs in runs.items():
            vals = [r["blocks_per_s"] for r in rs]
            print("# %-9s %9d  (%d .. %d)" % (arm, statistics.median(vals), min(vals), max(vals)))


if __name__ == "__main__":
    main()
