#!/usr/bin/env python3
"""Light tables (csrc/kernels_light.h) on the shape the same-MSM argument's prover would use, against the path such MSMs take today, in
ONE process on one GPU: the two sides alternate three times, a third of --reps (>= 20) repetitions each after a warm-up, and the median
of the three medians is kept for each side.

For P = 1, 8, 64 provers at n = 128: 2 n P = 256 P variable bases (vec_T | vec_U per prover), and per halving launch 4 P MSMs of 64
terms over them (L_T, L_U, R_T, R_U).  A proof has lg n + 1 = 8 such launches over the SAME bases, so

  build_ms        cg1_light_create + cg1_light_destroy: the upload, the allocation, k_light_chain, k_light_multiples, one wait
  light_ms        one cg1_light_msm call of 4 P MSMs x 64 terms (native level: indices and packed scalars in, 48-byte encodings out)
  yardstick_ms    the same sums through cg1_msm_batched (k_msm_small: what compute_MSM_batch runs), points and scalars in, blobs out
  proof           build_ms + 8 light_ms  against  8 yardstick_ms

The window plan is the loaded library's (CG1_LIGHT_WINDOW_BITS; an A/B library built with another width -- build.build_variant(path,
["-DCG1_LIGHT_WINDOW_BITS=5"]) -- is selected with CURDLE_G1_LIB=path).  Both sides are checked to give the same points first.

One run prints one JSON line.  `--summarize a.json b.json c.json [--label text]` reads three runs of one plan and prints the table with
the verdict per shape by the rule of tools/gpu_fixed_base_timing.py: FASTER when the light side's median lies below the yardstick's by
more than the spread (max - min) of the yardstick's own medians over the runs.

    python tools/gpu_light_table_timing.py [--reps 30] > run1.json
    python tools/gpu_light_table_timing.py --summarize run1.json run2.json run3.json
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
PROVERS = (1, 8, 64)
ROUNDS = 8                                                       # lg n + 1 launches per proof at n = 128


def median_ms(fn, reps):
    fn(); fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def summarize(paths, label):
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    r0 = runs[0]
    print("window plan: c = %d, %d windows, %d bytes per base%s" % (r0["window_bits"], r0["windows"], r0["bytes_per_base"], "   (%s)" % label if label else ""))
    print("%-22s %10s %10s %12s %10s | %12s %12s %8s  %s" % ("shape", "build ms", "light ms", "yardstick ms", "spread ms", "proof light", "proof yard", "ratio", "verdict (proof)"))
    for p in PROVERS:
        key = "provers_%d" % p
        b = [r["shapes"][key]["build_ms"] for r in runs]
        l = [r["shapes"][key]["light_ms"] for r in runs]
        y = [r["shapes"][key]["yardstick_ms"] for r in runs]
        pl = [bb + ROUNDS * ll for bb, ll in zip(b, l)]
        py = [ROUNDS * yy for yy in y]
        f, yard, spread = statistics.median(pl), statistics.median(py), max(py) - min(py)
        verdict = "FASTER" if f < yard - spread else ("slower" if f > yard + spread else "no difference")
        print("%-22s %10.3f %10.4f %12.4f %10.4f | %12.3f %12.3f %7.2fx  %s   (light runs: %s; yardstick runs: %s)" %
              ("%d x 4 MSMs x 64" % p, statistics.median(b), statistics.median(l), statistics.median(y), max(y) - min(y), f, yard, yard / f, verdict,
               " ".join("%.3f" % v for v in pl), " ".join("%.3f" % v for v in py)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--summarize", nargs="+")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.label)
    assert a.reps >= 20, "the medians are taken over at least 20 repetitions"
    sys.path.insert(0, ROOT)
    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    ctx = N.Context(0)
    windows = int(N.cg1_light_digits(bytes(32), (ctypes.c_int16 * 128)()))
    rng = random.Random(12)
    R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    out = {"reps": a.reps, "windows": windows, "window_bits": (256 + windows - 1) // windows, "shapes": {}}

    # 256 P distinct points: k_i G through the generator's table, affine96 on the device
    nmax = 256 * max(PROVERS)
    d_sc, d_pts = ctx.alloc(32 * nmax), ctx.alloc(96 * nmax)
    d_sc.upload(b"".join(rng.randrange(1, R).to_bytes(32, "little") for _ in range(nmax)))
    ctx.check(N.cg1_generator_mul_device(ctx.handle, d_sc.ptr, nmax, d_pts.ptr, None))
    pts96 = d_pts.download()
    d_sc.free(); d_pts.free()

    for p in PROVERS:
        nb = 256 * p
        raw = pts96[: 96 * nb]
        idx, offsets = [], [0]
        for q in range(p):                                       # L_T, L_U over the right halves, R_T, R_U over the left halves
            for lo in (64, 192, 0, 128):
                idx += list(range(256 * q + lo, 256 * q + lo + 64))
                offsets.append(len(idx))
        sc = b"".join(rng.randrange(R).to_bytes(32, "little") for _ in idx)
        term_pts = b"".join(raw[96 * i: 96 * i + 96] for i in idx)
        tab = ctx.light_table(raw, nb)
        out["bytes_per_base"] = tab.nbytes // nb
        light = lambda: ctx.light_msm_host(tab, idx, sc, offsets, compressed=True)
        yard = lambda: ctx.msm_batched_host(term_pts, sc, offsets)
        comp = ctypes.create_string_buffer(48 * (4 * p))
        N.cg1_batch_compress(comp, b"".join(yard()), 4 * p)
        assert b"".join(light()) == comp.raw, "the two paths disagree"
        l_ms, y_ms = [], []
        for _ in range(3):                                       # alternating, a third of the repetitions at a time
            l_ms.append(median_ms(light, max(a.reps // 3, 7)))
            y_ms.append(median_ms(yard, max(a.reps // 3, 7)))
        tab.free()

        def build():
            t = ctx.light_table(raw, nb)
            t.free()
        out["shapes"]["provers_%d" % p] = {"build_ms": median_ms(build, max(a.reps // 3, 7)), "light_ms": statistics.median(l_ms),
                                           "yardstick_ms": statistics.median(y_ms)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
