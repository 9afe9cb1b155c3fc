#!/usr/bin/env python3
"""The tracker scan -- which of T trackers do V secrets open -- from host bytes to the bitmap: tracker_scan.TrackerScanner.scan_packed on
the device (cg1_tracker_match_device, csrc/kernels_tracker_scan.h) against what the library offered for the job without it.

  scan        TrackerScanner(device=True).scan_packed: bytes in, bitmap out, one native call
  composed    the trackers split and decoded unchecked (cg1_batch_decompress_device), a replicated V * T scalar array uploaded,
              cg1_batch_mul_device over V * T outputs (k_batch_mul: a double-and-add ladder per pair and an affine finish), the
              V * T x 96-byte result brought back and compared with the decoded k_r_G in numpy
  tables, ladders   further lines for V <= 64, not sides of the verdict: the same scan with the device call's route forced (context
              parameter "tracker_scan_ladder_max_ks" = 0: the light tables whatever V is; = 1024: one ladder per pair) -- where the
              two meet is the crossover the default rule (CG1_TRACKER_MATCH_LADDER_MAX_KS secrets) stands on
  host        a further line for the small shapes only (V * T <= HOST_PAIRS_MAX): the host twin, cg1_tracker_match on the worker pool

Shapes: T = 8 192 with V = 1, 8, 64, 1 024, 16 384, and T = 16 384 with V = 1 024; and T = 8 192 with V = 16, 32 for the crossover.
Where V * T exceeds SLICE_OUTPUTS the composed side runs the largest whole number of secrets that fits (SLICE_OUTPUTS / T of them) and its time is SCALED by V / that number -- the JSON
says so per shape ("composed_scaled_from") -- because 2^27 outputs are 12.9 GB of results and 4.3 GB of scalars.

The sides run in ONE process and ALTERNATE call by call; the figure is the median wall time of the Python call over --reps (>= 30)
repetitions after two warm-ups.  Before anything is timed the verdicts are compared bit for bit: the scan's bitmap against the composed
side's over the composed slice, and against the matches planted when the inputs were made over the whole matrix.  Then five more scans
run with the context parameter "tracker_scan_timing" = 1, in which the call waits between its phases: the medians of the table
builds (k_light_chain, k_light_multiples, k_tracker_normalise over all tiles) and of the match kernels are reported separately.

    python tools/gpu_tracker_scan_timing.py [--reps 30] > run1.json
    python tools/gpu_tracker_scan_timing.py --summarize run1.json run2.json run3.json
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8192, 1), (8192, 8), (8192, 16), (8192, 32), (8192, 64), (8192, 1024), (8192, 16384), (16384, 1024)]
ROUTES_MAX_KS = 64
DEFAULT_LADDER_MAX_KS = 32                 # CG1_TRACKER_MATCH_LADDER_MAX_KS (include/curdle_g1.h)
SLICE_OUTPUTS = 1 << 21
HOST_PAIRS_MAX = 1 << 16


def summarize(paths):
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    print("%-16s %10s %12s %10s %8s  %-13s %9s %9s %9s %9s %9s  %s" % ("T x V", "scan ms", "composed ms", "spread ms", "ratio", "verdict", "build ms", "match ms", "tables ms",
                                                                      "ladders ms", "host ms", "composed side"))
    for T, V in SHAPES:
        s = "%d x %d" % (T, V)
        med = lambda key: [r["shapes"][s][key] for r in runs]
        ys, fs = med("composed_ms"), med("scan_ms")
        y, spread, f = statistics.median(ys), max(ys) - min(ys), statistics.median(fs)
        verdict = "FASTER" if f < y - spread else ("slower" if f > y + spread else "no difference")
        opt = lambda key: (lambda v: "%.3f" % statistics.median(v) if v else "-")([v for v in med(key) if v is not None])
        sc = runs[0]["shapes"][s]["composed_scaled_from"]
        print("%-16s %10.3f %12.3f %10.3f %7.2fx  %-13s %9.3f %9.3f %9s %9s %9s  %s   (scan runs: %s; composed runs: %s)" %
              (s, f, y, spread, y / f, verdict, statistics.median(med("build_ms")), statistics.median(med("match_ms")), opt("tables_ms"), opt("ladders_ms"), opt("host_ms"), "measured whole" if sc == V else "%d secrets measured, scaled x %g" % (sc, V / sc),
               " ".join("%.3f" % v for v in fs), " ".join("%.3f" % v for v in ys)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--summarize", nargs="+")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    assert a.reps >= 30, "the medians are taken over at least 30 repetitions"
    sys.path.insert(0, ROOT)
    import numpy as np

    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd.opening_prover import generator_multiples
    from curdleproofs_pie_amd.shuffle_verifier import FR_MODULUS as R
    from curdleproofs_pie_amd.tracker_scan import TrackerScanner

    ctx = N.default_context()
    scanner = TrackerScanner(ctx, device=True)
    host_scanner = TrackerScanner(device=False)
    rng = random.Random(16)
    out = {"reps": a.reps, "slice_outputs": SLICE_OUTPUTS, "shapes": {}}
    for T, V in SHAPES:
        # honest trackers r_G = r G, k_r_G = (r k) G; every 512th tracker is opened by one of the secrets, the others by nobody's
        ks = [rng.randrange(1, R) for _ in range(V)]
        rs = [rng.randrange(1, R) for _ in range(T)]
        planted = {i: (i // 512 * 7) % V for i in range(0, T, 512)}
        opener = [ks[planted[i]] if i in planted else rng.randrange(1, R) for i in range(T)]
        rG = generator_multiples(rs, ctx, device=True)
        krG = generator_multiples([r * k % R for r, k in zip(rs, opener)], ctx, device=True)
        trackers96 = b"".join(r + s for r, s in zip(rG, krG))
        ks32 = b"".join(k.to_bytes(32, "little") for k in ks)
        words = (V + 63) // 64
        want = np.zeros((T, words), dtype=np.uint64)
        for i, j in planted.items():
            want[i, j >> 6] |= np.uint64(1 << (j & 63))

        Vs = V if T * V <= SLICE_OUTPUTS else SLICE_OUTPUTS // T
        wire = b"".join(rG) + b"".join(krG)
        d_in, d_aff, d_st = ctx.alloc(96 * T), ctx.alloc(192 * T), ctx.alloc(2 * T)
        d_sc, d_out = ctx.alloc(32 * T * Vs), ctx.alloc(96 * T * Vs)

        def composed():
            d_in.upload(wire)
            ctx.check(N.cg1_batch_decompress_device(ctx.handle, d_in.ptr, d_aff.ptr, d_st.ptr, 2 * T, 0))
            d_sc.upload(b"".join(ks32[32 * j: 32 * j + 32] * T for j in range(Vs)))           # scalars[j * T + i] = k_j
            ctx.check(N.cg1_batch_mul_device(ctx.handle, d_aff.ptr, T, d_sc.ptr, d_out.ptr, T * Vs))
            got = np.frombuffer(d_out.download(96 * T * Vs), dtype=np.uint8).reshape(Vs, T, 96)
            s_aff = np.frombuffer(d_aff.download(96 * T, 96 * T), dtype=np.uint8).reshape(T, 96)
            ok = np.frombuffer(d_st.download(2 * T), dtype=np.uint8).reshape(2, T).max(axis=0) == 0
            return (got == s_aff[None, :, :]).all(axis=2) & ok[None, :]                           # [j, i]

        def scan():
            return scanner.scan_packed(trackers96, ks32)

        bitmap, tst, kst = scan()
        assert not any(tst) and not any(kst)
        got = np.frombuffer(bitmap, dtype="<u8").reshape(T, words)
        assert (got == want).all(), "the scan's bitmap is not the planted matrix"
        verdict = composed()
        bits = ((got[:, None, :Vs // 64 + 1] >> np.arange(64, dtype=np.uint64)[None, :, None]) & np.uint64(1)).astype(bool)      # [i, bit, word]
        mine = bits.transpose(2, 1, 0).reshape(-1, T)[:Vs]                                        # [j, i]
        assert (mine == verdict).all(), "the scan and the composed path disagree"
        fns = {"scan": scan, "composed": composed}
        with_host = T * V <= HOST_PAIRS_MAX
        if V <= ROUTES_MAX_KS:
            def forced(max_ks):
                def run():
                    ctx.set_param("tracker_scan_ladder_max_ks", max_ks)
                    try:
                        return scan()
                    finally:
                        ctx.set_param("tracker_scan_ladder_max_ks", DEFAULT_LADDER_MAX_KS)
                return run
            fns["tables"], fns["ladders"] = forced(0), forced(1024)
            assert fns["tables"]()[0] == bitmap and fns["ladders"]()[0] == bitmap
        if with_host:
            fns["host"] = lambda: host_scanner.scan_packed(trackers96, ks32)
            assert fns["host"]()[0] == bitmap
        samples = {side: [] for side in fns}
        for rep in range(a.reps + 2):                                    # two warm-ups, then the sides alternate
            for side, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= 2:
                    samples[side].append(dt)
        ctx.set_param("tracker_scan_timing", 1)
        phases = []
        ms = (ctypes.c_float * 2)()
        for _ in range(5):
            scan()
            ctx.check(N.cg1_tracker_match_last_ms(ctx.handle, ms))
            phases.append((ms[0], ms[1]))
        ctx.set_param("tracker_scan_timing", 0)
        for b in (d_in, d_aff, d_st, d_sc, d_out):
            b.free()
        out["shapes"]["%d x %d" % (T, V)] = {
            "scan_ms": statistics.median(samples["scan"]), "composed_ms": statistics.median(samples["composed"]) * (V / Vs), "composed_scaled_from": Vs,
            "host_ms": statistics.median(samples["host"]) if with_host else None,
            "tables_ms": statistics.median(samples["tables"]) if "tables" in samples else None,
            "ladders_ms": statistics.median(samples["ladders"]) if "ladders" in samples else None,
            "build_ms": statistics.median(p[0] for p in phases), "match_ms": statistics.median(p[1] for p in phases)}
        print("%d x %d done" % (T, V), out["shapes"]["%d x %d" % (T, V)], file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
