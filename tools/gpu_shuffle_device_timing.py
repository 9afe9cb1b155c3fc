#!/usr/bin/env python3
"""A whole shuffle proof proved on the device in one native call (prover_kernels.shuffle_prove_device_many, csrc/capi_shuffle.h) against
the best path without it, at (ell, n_blinders) = (124, 4) for 1, 8 and 64 provers in step: CurdleProofsProof.new after
shuffle_permute_and_commit_input, inputs as Python objects in, CurdleProofsProof.to_bytes() per prover out.

  device      shuffle_prove_device_many: one native call per batch, no Python between the arguments
  composed    the yardstick: curdleproofs.py:63-149 written out in Python over the three existing device provers -- the head transcript on the
              host, A for all provers by ONE table.msm_many, then same_permutation_prove_device_many, same_scalar_prove_device_many and
              same_msm_prove_device_many, the bytes assembled from their results
  lazy        a second line, not a side of the verdict: the reference's unchanged control flow over the deferred G1Point operators, one
              proof at a time (tools/replay_call_trace.py, the recorded call sequence of one ell = 124 proof)

The two sides run in ONE process and ALTERNATE call by call; the figure is the median wall time of the Python call over --reps (>= 30)
repetitions after two warm-ups.  Both sides must produce the same bytes (checked once per shape, before anything is timed).  One run
prints one JSON line.

`--summarize a.json b.json c.json` prints the table over three runs: a shape counts as FASTER when the device median (the median of
the runs) lies below the yardstick's by more than the spread (max - min) of the yardstick's own medians.

`--target P` is a short target for `rocprofv3 --kernel-trace --stats`: five device calls for P provers and nothing else;
`--trace-summary kernel_trace.csv` then prints, for the LAST call of the trace, every kernel's time and the gap before it -- the gaps in
front of k_same_perm_begin and of the same-MSM chain's first k_table_msm are the two host waits, and what runs inside them is the device
work queued under the host's hashing.

    python tools/gpu_shuffle_device_timing.py [--reps 30] > run1.json
    python tools/gpu_shuffle_device_timing.py --summarize run1.json run2.json run3.json
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/gpu_shuffle_device_timing.py --target 8
    python tools/gpu_shuffle_device_timing.py --trace-summary out/*/*_kernel_trace.csv
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, "shuffle_124_1_prover"), (8, "shuffle_124_8_provers"), (64, "shuffle_124_64_provers")]
SIDES = ("device", "composed")
NB = 4


def summarize(paths):
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    print("%-26s %10s %12s %10s %8s  %s" % ("shape", "device ms", "composed ms", "spread ms", "ratio", "verdict"))
    for _, s in SHAPES:
        med = {side: [r["shapes"][s][side + "_ms"] for r in runs] for side in SIDES}
        ys = med["composed"]
        y, spread, f = statistics.median(ys), max(ys) - min(ys), statistics.median(med["device"])
        verdict = "FASTER" if f < y - spread else ("slower" if f > y + spread else "no difference")
        print("%-26s %10.4f %12.4f %10.4f %7.2fx  %s   (device runs: %s; composed runs: %s)" %
              (s, f, y, spread, y / f, verdict, " ".join("%.4f" % v for v in med["device"]), " ".join("%.4f" % v for v in ys)))
    print("the unchanged lazy prover, one proof at a time (replayed call sequence, ell = 124): %s ms" % " ".join("%.3f" % r["lazy_prove_ms"] for r in runs))


def trace_summary(path):
    import csv

    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    short = lambda n: n.split("(")[0].split("<")[0].split("::")[-1]
    begins = [i for i, r in enumerate(rows) if "k_shuffle_begin" in r["Kernel_Name"]]
    call = rows[begins[-1]:]
    t0 = int(call[0]["Start_Timestamp"])
    print("the last call of %s: %d launches, %.1f us from the first kernel's start to the last one's end" %
          (os.path.basename(path), len(call), (int(call[-1]["End_Timestamp"]) - t0) / 1e3))
    print("%4s %-20s %10s %10s %10s" % ("#", "kernel", "start us", "time us", "gap us"))
    prev_end = None
    for i, r in enumerate(call):
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        gap = 0.0 if prev_end is None else (s - prev_end) / 1e3
        print("%4d %-20s %10.1f %10.1f %10.1f" % (i, short(r["Kernel_Name"]), (s - t0) / 1e3, (e - s) / 1e3, gap))
        prev_end = e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--summarize", nargs="+")
    ap.add_argument("--target", type=int, default=0, help="five device calls for that many provers (a target for rocprofv3)")
    ap.add_argument("--trace-summary")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    if a.trace_summary:
        return trace_summary(a.trace_summary)
    assert a.reps >= 30 or a.target, "the medians are taken over at least 30 repetitions"
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd import msm_accumulator as M
    from curdleproofs_pie_amd import prover_kernels as K
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.py_arkworks_bls12381 import CURVE_ORDER as R, G1Point, Scalar, points_to_affine96

    rng = random.Random(29)
    ell, n = 124, 124 + NB
    rs = lambda: Scalar(rng.randint(1, R - 1))
    vec = lambda m: [rs() for _ in range(m)]
    comp = lambda p: bytes(p.to_compressed_bytes())
    fr32 = lambda s: bytes(s.to_le_bytes())
    base = [G1Point.from_compressed_bytes(comp(p)) for p in M.batch_mul([G1Point()] * (n + 3), vec(n + 3))]
    crs = types.SimpleNamespace(vec_G=base[:ell], vec_H=base[ell:n], H=base[n], G_t=base[n + 1], G_u=base[n + 2])
    tab = FixedBaseTable(base)
    Z1 = G1Point.identity()
    G_m = crs.vec_G + crs.vec_H[:2] + [crs.G_t, crs.G_u]

    def flat(res):
        out = b""
        for f in res:
            if isinstance(f, tuple):
                out += flat(f)
            else:
                for v in f if isinstance(f, list) else [f]:
                    out += comp(v) if hasattr(v, "to_compressed_bytes") else fr32(v)
        return out

    def composed(provers):
        ts, vas, aps = [], [], []
        for _, vR, vS, vT, vU, M_, perm, k, mbl, dr in provers:
            t = CurdleproofsTranscript(b"curdleproofs")
            t.append_list(b"curdleproofs_step1", [comp(p) for p in vR + vS + vT + vU])
            t.append(b"curdleproofs_step1", comp(M_))
            va = t.get_and_append_challenges(b"curdleproofs_vec_a", ell)
            ts.append(t); vas.append(va); aps.append([va[j] for j in perm])
        zero = Scalar(0)
        As = tab.msm_many([(crs.vec_G + crs.vec_H, ap + list(pr[9][0]) + [zero, zero]) for ap, pr in zip(aps, provers)])
        sp = K.same_permutation_prove_device_many(tab, [(crs.vec_G, crs.vec_H, crs.H, A, pr[5], va, pr[6], list(pr[9][0]) + [zero, zero], pr[8], pr[9][1], pr[9][2], pr[9][3])
                                                        for A, va, pr in zip(As, vas, provers)], ts)
        ss = K.same_scalar_prove_device_many(tab, [(crs.G_t, crs.G_u, crs.H, pr[1], pr[2], va, pr[7], *pr[9][4:9]) for va, pr in zip(vas, provers)], ts)
        sm = K.same_msm_prove_device_many(tab, [(G_m, A + s[2][0] + s[3][0], s[2][1], s[3][1], pr[3] + [Z1, Z1, crs.H, Z1], pr[4] + [Z1, Z1, Z1, crs.H],
                                                 ap + list(pr[9][0]) + [pr[9][4], pr[9][5]], pr[9][9]) for A, s, ap, pr in zip(As, ss, aps, provers)], ts)
        out = []
        for A, p_, s, m in zip(As, sp, ss, sm):
            R_, S_, cm_T, cm_U, cm_A, cm_B, z_k, z_t, z_u = s
            out.append(comp(A) + flat((cm_T, cm_U, R_, S_)) + flat(p_) + flat((cm_A, cm_B, z_k, z_t, z_u)) + flat(m))
        return out

    def device(provers):
        return K.shuffle_prove_device_many(tab, provers)

    out = {"reps": a.reps, "ell": ell, "shapes": {}}
    for P, name in (SHAPES if not a.target else [(a.target, "target")]):
        pts = [G1Point.from_compressed_bytes(comp(p)) for p in M.batch_mul([G1Point()] * (2 * ell * P), vec(2 * ell * P))]      # carry their certificate
        provers = []
        for p in range(P):
            vR, vS = pts[2 * ell * p: 2 * ell * p + ell], pts[2 * ell * p + ell: 2 * ell * (p + 1)]
            perm = list(range(ell))
            rng.shuffle(perm)
            k, mbl = rs(), vec(NB)
            both = M.batch_mul_same_scalar(vR + vS, k)
            both = [G1Point.from_compressed_bytes_unchecked(comp(x)) for x in both]
            vT, vU = [both[j] for j in perm], [both[ell + j] for j in perm]
            M_ = tab.msm([Scalar(j) for j in perm] + mbl, crs.vec_G + crs.vec_H)
            M_ = G1Point.from_compressed_bytes_unchecked(comp(M_))
            provers.append((crs, vR, vS, vT, vU, M_, perm, k, mbl, (vec(2), vec(NB), vec(n), vec(n - 2), *vec(5), vec(n))))
        points_to_affine96([x for pr in provers for v in pr[1:5] for x in v])      # normalised once, outside the timed region, for both sides
        if a.target:
            for _ in range(5):
                device(provers)
            tab.close()
            return
        fns = {"device": device, "composed": composed}
        assert device(provers) == composed(provers), name                # the bytes are compared first
        samples = {side: [] for side in SIDES}
        for rep in range(a.reps + 2):                                    # two warm-ups, then the sides alternate
            for side in SIDES:
                t0 = time.perf_counter()
                fns[side](provers)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= 2:
                    samples[side].append(dt)
        out["shapes"][name] = {side + "_ms": statistics.median(samples[side]) for side in SIDES}
    tab.close()
    import replay_call_trace

    out["lazy_prove_ms"] = replay_call_trace.measure(reps=5, ab=False)["prove_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
