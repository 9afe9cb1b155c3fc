#!/usr/bin/env python3
"""A chain of Whisk shuffles PROVED over a device-resident tracker set (shuffle_chain.ShuffleChainProver) against the only path there was
for the same index lists, and against the ceiling.

Workload: ell = 124, a set of 16 384 trackers, --blocks (1 024) blocks; every block names 124 distinct pseudo-random slots, with NO
restriction between blocks: nearly every block reads slots its predecessors wrote.

  chain        ShuffleChainProver.prove_blocks_packed over all blocks in one call; the set is put back to its initial state before every
               pass, outside the clock.  Also reported from last_stats: the tracker stage alone (certification, lineage, the one
               k_chain_lineage_mul launch, the scatter: hipEvents on the stream), the distinct slots certified, and the share of the native
               call outside cg1_shuffle_prove_device
  flush        ShuffleBatchProver.generate_packed over a model of the set, the pending blocks flushed whenever a block touches a slot a
               pending block wrote (tests/test_shuffle_chain_gpu.py::Kit.chain): what a caller had to do before
  independent  generate_packed over the same number of INDEPENDENT lists (every block reads the initial set) in its groups of 64: the ceiling

`chain` and `flush` must agree byte for byte (posts, proofs, the final set): their digests are compared.  Every arm is a process of its own;
the arms alternate for --rounds rounds; each process warms up on a prefix of the blocks and times --passes passes (wall clock around calls
that end in host bytes).  ms per block = median pass time / blocks.

    python tools/gpu_chain_prove_timing.py [--blocks 1024] [--rounds 3] [--passes 2] > profiles/r21_chain_prove_timing.txt
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELL, NB, SLOTS = 124, 4, 16384


def make_workload(path, blocks, seed):
    import ctypes
    import random

    import numpy as np

    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
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

    enc = multiples_of_g(ELL + NB + 3)
    initial = multiples_of_g(2 * SLOTS)
    nprng = np.random.default_rng(seed)
    idx = np.stack([nprng.permutation(SLOTS)[:ELL] for _ in range(blocks)]).astype("<u4")      # distinct inside a block, unrestricted between blocks
    np.savez(path, crs=np.frombuffer(enc, dtype=np.uint8), initial=np.frombuffer(initial, dtype=np.uint8), idx=idx)
    touched = np.zeros(SLOTS, dtype=bool)
    dependent = 0
    for b in range(blocks):
        dependent += bool(touched[idx[b]].any())
        touched[idx[b]] = True
    print(json.dumps({"blocks": blocks, "blocks_reading_an_earlier_write": dependent, "distinct_slots": int(touched.sum())}), flush=True)


def run_arm(arm, path, passes, seed):
    import types

    import numpy as np

    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point
    from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver

    w = np.load(path)
    enc, initial, idx = w["crs"].tobytes(), w["initial"].tobytes(), w["idx"]
    n, m = len(idx), ELL + NB
    pts = [G1Point.from_compressed_bytes_unchecked(enc[48 * i: 48 * i + 48]) for i in range(m + 3)]
    crs = types.SimpleNamespace(vec_G=pts[:ELL], vec_H=pts[ELL:m], H=pts[m], G_t=pts[m + 1], G_u=pts[m + 2])
    table = FixedBaseTable(pts)
    seed32 = bytes([seed % 256]) * 32
    res = {"arm": arm, "blocks": n, "hw_queues": N.hw_queues()}
    times, digest = [], None

    def flush_prove(prover, count):
        """the first `count` blocks over a model of the set: a generate_packed call whenever a block touches a pending write"""
        state = np.frombuffer(initial, dtype=np.uint8).reshape(SLOTS, 96).copy()
        posts, proofs, calls = [], [], 0
        pending, dirty, first = [], np.zeros(SLOTS, dtype=bool), 0

        def flush():
            nonlocal pending, first, calls
            if not pending:
                return
            rows = np.stack(pending)
            post, prf, st = prover.generate_packed(state[rows].tobytes(), seed=seed32, first_index=first)
            assert st == [0] * len(pending)
            post_rows = np.frombuffer(post, dtype=np.uint8).reshape(len(pending), ELL, 96)
            for r, p in zip(rows, post_rows):
                state[r] = p
            posts.append(post); proofs.append(prf)
            first += len(pending)
            calls += 1
            pending = []
            dirty[:] = False

        for b in range(count):
            if dirty[idx[b]].any():
                flush()
            pending.append(idx[b])
            dirty[idx[b]] = True
        flush()
        return b"".join(posts), b"".join(proofs), state.tobytes(), calls

    if arm == "chain":
        from curdleproofs_pie_amd.shuffle_chain import ShuffleChainProver, TrackerSet

        ts = TrackerSet(initial, N.Context(0))
        pr = ShuffleChainProver(crs, ts, table=table)
        pr.prove_blocks_packed(idx[:64].reshape(-1), 64, seed=seed32)                              # warm-up: a full group
        stats = []
        for p in range(passes):
            ts.replace(initial)
            t0 = time.perf_counter()
            post, proofs, st = pr.prove_blocks_packed(idx.reshape(-1), n, seed=seed32)
            times.append(time.perf_counter() - t0)
            assert st == [0] * n
            stats.append(dict(pr.last_stats))
            digest = hashlib.sha256(post + proofs + ts.packed()).hexdigest()
        med = lambda k: statistics.median(s[k] for s in stats)
        res.update(stage_ms=round(med("stage_ms"), 3), certified_slots=stats[-1]["certified_slots"], native_call_ms=round(med("call_ms"), 2),
                   in_shuffle_prove_device_ms=round(med("chain_ms"), 2), share_outside_shuffle_prove_device=round(1 - med("chain_ms") / med("call_ms"), 4))
    elif arm == "flush":
        prover = ShuffleBatchProver(crs, table=table)
        flush_prove(prover, 8)
        for p in range(passes):
            t0 = time.perf_counter()
            post, proofs, final, calls = flush_prove(prover, n)
            times.append(time.perf_counter() - t0)
            digest = hashlib.sha256(post + proofs + final).hexdigest()
        res.update(generate_packed_calls=calls)
    else:
        prover = ShuffleBatchProver(crs, table=table)
        state = np.frombuffer(initial, dtype=np.uint8).reshape(SLOTS, 96)
        pre = state[idx].tobytes()
        prover.generate_packed(pre[: 64 * ELL * 96], seed=seed32)
        for p in range(passes):
            t0 = time.perf_counter()
            post, proofs, st = prover.generate_packed(pre, seed=seed32)
            times.append(time.perf_counter() - t0)
            assert st == [0] * n
    res.update(pass_s=[round(t, 4) for t in times], ms_per_block=round(1e3 * statistics.median(times) / n, 4), digest=digest)
    table.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--arm", choices=("make", "chain", "flush", "independent"))
    ap.add_argument("--workload")
    a = ap.parse_args()
    if a.arm:
        sys.path.insert(0, ROOT)
        return make_workload(a.workload, a.blocks, a.seed) if a.arm == "make" else run_arm(a.arm, a.workload, a.passes, a.seed)
    with tempfile.TemporaryDirectory(prefix="chain_prove_timing_") as td:
        path = os.path.join(td, "workload.npz")

        def child(arm):
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--workload", path, "--blocks", str(a.blocks), "--passes", str(a.passes), "--seed", str(a.seed)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if done.returncode:
                sys.exit("arm %s failed (%d):\n%s" % (arm, done.returncode, done.stderr[-4000:]))
            return json.loads(done.stdout.strip().splitlines()[-1])

        print("# ell = %d over %d slots, unrestricted pseudo-random indices, distinct inside a block; %s" % (ELL, SLOTS, json.dumps(child("make"))), flush=True)
        runs = {"chain": [], "flush": [], "independent": []}
        for rnd in range(a.rounds):                          # the arms alternate
            for arm in runs:
                r = child(arm)
                runs[arm].append(r)
                print(json.dumps(r), flush=True)
        same = {r["digest"] for r in runs["chain"] + runs["flush"]}
        print("# chain and flush agree byte for byte (posts, proofs, final set): %s" % (len(same) == 1))
        print("# ms per block, median of the rounds' medians (min .. max over rounds)")
        for arm, rs in runs.items():
            vals = [r["ms_per_block"] for r in rs]
            print("# %-12s %9.4f  (%.4f .. %.4f)" % (arm, statistics.median(vals), min(vals), max(vals)))
        c = runs["chain"]
        print("# chain: tracker stage %.3f ms (median), %d distinct slots certified, %.1f %% of the native call outside cg1_shuffle_prove_device" % (
            statistics.median(r["stage_ms"] for r in c), c[-1]["certified_slots"], 100 * statistics.median(r["share_outside_shuffle_prove_device"] for r in c)))
        if len(same) != 1:
            sys.exit("the arms disagree")


if __name__ == "__main__":
    main()
