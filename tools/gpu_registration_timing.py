#!/usr/bin/env python3
"""Whisk registrations in bulk (registration.RegistrationBatchMaker, cg1_whisk_register_device) against the only route there was, and the
A/B of the two candidate kernels for the five multiples of G.  From k bytes to output bytes, everything a caller pays inside the clock.

  make            RegistrationBatchMaker(device=True).make_packed(ks32, seed=...), also at 16 .. 512 items
  host            the same call on the host twin (device=False), up to --host-max items: where the two meet is the threshold of device=None
  composed        what a caller had to do before: r and b by hashlib (the same derivation), k r mod FR_MODULUS in Python,
                  generator_multiples twice (r_G, k_r_G), then OpeningBatchProver.prove_packed with the blinders -- which decodes the tracker
                  it was just handed and runs a ladder for B.  Its bytes must equal `make`'s: the digests are compared
  points_shared   the device stage of the five multiples alone (cg1_whisk_register_points_device): k_register_points, one lane and ONE
                  inversion per item
  points_single   the same stage by k_generator_mul over the 5 n scalars: one lane and one inversion per POINT.  The two must agree byte for byte

Every arm is a process of its own; the arms alternate for --rounds rounds; a process warms up once per size and times --passes passes
(wall clock around calls that end in host bytes, or in a finished stream for the two stage arms); ms = median pass.  Every child runs under
its own time limit and the first failure ends the run.

    python tools/gpu_registration_timing.py [--sizes 1024,65536,1048576] [--rounds 3] [--passes 2] > profiles/r22_registration_timing.txt
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SMALL = (16, 32, 64, 128, 256, 512)


def secrets_for(n, seed):
    """n x 32 bytes below 2^254 (< FR_MODULUS): pseudo-random, made outside every clock"""
    import numpy as np

    a = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x3F
    return a.tobytes()


def run_arm(arm, sizes, passes, seed, host_max):
    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd import opening_prover as P
    from curdleproofs_pie_amd import registration as G

    seed32 = hashlib.sha256(b"registration timing %d" % seed).digest()
    res = {"arm": arm, "hw_queues": N.hw_queues(), "sizes": {}}
    ctx = N.default_context() if arm != "host" else None

    def composed(ks32, n):
        draws = [G.registration_draws_from_seed(seed32, i) for i in range(n)]
        ks = [int.from_bytes(ks32[32 * i: 32 * i + 32], "little") for i in range(n)]
        r_G = P.generator_multiples([r for r, _ in draws], ctx, device=True)
        k_r_G = P.generator_multiples([k * r % R for k, (r, _) in zip(ks, draws)], ctx, device=True)
        trk = b"".join(a + b for a, b in zip(r_G, k_r_G))
        proofs, kcs, st = P.OpeningBatchProver(ctx, device=True).prove_packed(trk, ks32, b"".join(b.to_bytes(32, "little") for _, b in draws))
        return trk, kcs, proofs, st

    for n in sizes:
        if arm == "host" and n > host_max:
            continue
        if arm in ("make", "host") or arm == "composed":
            ks32 = secrets_for(n, seed + n)
            maker = G.RegistrationBatchMaker(ctx, device=(arm == "make"))
            call = (lambda: composed(ks32, n)) if arm == "composed" else (lambda: maker.make_packed(ks32, seed=seed32))
            out = call()                                           # warm-up: tables, kept buffers
            assert list(out[3]) == [0] * n
            times = []
            for _ in range(passes):
                t0 = time.perf_counter()
                out = call()
                times.append(time.perf_counter() - t0)
            digest = hashlib.sha256(out[0] + out[1] + out[2]).hexdigest()
        else:
            sc = secrets_for(5 * n, seed + n)
            d_sc, d_out = ctx.alloc(160 * n), ctx.alloc(240 * n)
            d_sc.upload(sc)
            shared = 1 if arm == "points_shared" else 0
            ctx.check(N.cg1_whisk_register_points_device(ctx.handle, d_sc.ptr, n, d_out.ptr, shared))
            times = []
            for _ in range(passes):
                t0 = time.perf_counter()
                ctx.check(N.cg1_whisk_register_points_device(ctx.handle, d_sc.ptr, n, d_out.ptr, shared))
                times.append(time.perf_counter() - t0)
            digest = hashlib.sha256(d_out.download(240 * n)).hexdigest()
            d_sc.free()
            d_out.free()
        res["sizes"][str(n)] = {"ms": round(1e3 * statistics.median(times), 4), "pass_ms": [round(1e3 * t, 4) for t in times], "digest": digest}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--host-max", type=int, default=1024)
    ap.add_argument("--stage-sizes", default="8192,16384,32768,49152", help="further sizes for the two stage arms alone: where the two kernels cross")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--arm", choices=("make", "host", "composed", "points_shared", "points_single"))
    a = ap.parse_args()
    big = [int(s) for s in a.sizes.split(",") if s]
    if a.arm:
        sys.path.insert(0, ROOT)
        return run_arm(a.arm, big, a.passes, a.seed, a.host_max)
    stage = sorted(set(big) | {int(s) for s in a.stage_sizes.split(",") if s})
    sizes = {"make": sorted(set(SMALL) | set(big)), "host": sorted(set(SMALL) | {n for n in big if n <= a.host_max}), "composed": big, "points_shared": stage,
             "points_single": stage}

    def child(arm):
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--sizes", ",".join(map(str, sizes[arm])), "--passes", str(a.passes), "--seed", str(a.seed),
               "--host-max", str(a.host_max)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("arm %s passed its time limit of %d s: nothing more is started" % (arm, a.child_timeout))
        if done.returncode:
            sys.exit("arm %s failed (%d): nothing more is started\n%s" % (arm, done.returncode, done.stderr[-4000:]))
        return json.loads(done.stdout.strip().splitlines()[-1])

    runs = {arm: [] for arm in sizes}
    for rnd in range(a.rounds):                              # the arms alternate
        for arm in runs:
            r = child(arm)
            runs[arm].append(r)
            print(json.dumps(r), flush=True)

    def med(arm, n):
        vals = [r["sizes"][str(n)]["ms"] for r in runs[arm] if str(n) in r["sizes"]]
        return (statistics.median(vals), min(vals), max(vals)) if vals else None

    def digests(arms, n):
        return {r["sizes"][str(n)]["digest"] for arm in arms for r in runs[arm] if str(n) in r["sizes"]}

    print("# ms per call, median of the rounds' medians (min .. max over rounds)")
    for arm in runs:
        for n in sizes[arm]:
            m = med(arm, n)
            print("# %-14s n = %8d  %12.4f  (%.4f .. %.4f)  %.3f us per item" % (arm, n, m[0], m[1], m[2], 1e3 * m[0] / n))
    agree = all(len(digests(("make", "composed", "host"), n)) == 1 for n in big) and all(len(digests(("points_shared", "points_single"), n)) == 1 for n in stage)
    print("# make, composed and host agree byte for byte, and so do the two stage kernels: %s" % agree)
    for n in big:
        print("# n = %8d: composed / make = %.2f" % (n, med("composed", n)[0] / med("make", n)[0]))
    for n in stage:
        print("# n = %8d: points_single / points_shared = %.2f" % (n, med("points_single", n)[0] / med("points_shared", n)[0]))
    both = [n for n in sizes["host"] if med("host", n)[0] > med("make", n)[0]]
    print("# the host twin is slower than the device call from n = %s on" % (both[0] if both else "(never, up to %d)" % a.host_max))
    if not agree:
        sys.exit("the arms disagree")


if __name__ == "__main__":
    main()
