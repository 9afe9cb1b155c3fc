#!/usr/bin/env python3
"""GenerateWhiskShuffleProof for a batch, from tracker bytes to post-tracker bytes and M || proof, at (ell, n_blinders) = (124, 4) for 1,
8 and 64 shuffles in step: shuffle_prover.ShuffleBatchProver.prove_many (one native call, csrc/capi_whisk_shuffle.h) against the path
without it.

  batched     ShuffleBatchProver.prove_many: bytes in, bytes out
  snippet     the yardstick, INTEGRATION section 3k as written, per shuffle: the 2 ell trackers decoded CHECKED into G1Points,
              shuffle_permute_and_commit_input(..., table=) -- one same-scalar launch and one table MSM each --, then ONE
              shuffle_prove_device_many for all shuffles, then M and the 2 ell post-tracker points compressed
  front       a second line, not a side of the verdict: cg1_whisk_shuffle_front alone (Context.whisk_shuffle_front)

The two sides run in ONE process and ALTERNATE call by call; the figure is the median wall time of the Python call over --reps (>= 30)
repetitions after two warm-ups.  Both sides must produce the same bytes (checked once per shape, before anything is timed): the
yardstick draws its vec_m_blinders from `random`, which is seeded before each of its calls, and the batched side is handed the same
values.  One run prints one JSON line.

`--summarize a.json b.json c.json` prints the table over three runs: a shape counts as FASTER when the batched median (the median of
the runs) lies below the yardstick's by more than the spread (max - min) of the yardstick's own medians.

`--target P` is a short target for `rocprofv3 --kernel-trace --stats`: five batched calls for P shuffles and nothing else;
`--trace-summary kernel_trace.csv` then prints what the front's kernels took in the LAST call of the trace.

    python tools/gpu_whisk_shuffle_prover_timing.py [--reps 30] > run1.json
    python tools/gpu_whisk_shuffle_prover_timing.py --summarize run1.json run2.json run3.json
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/gpu_whisk_shuffle_prover_timing.py --target 64
    python tools/gpu_whisk_shuffle_prover_timing.py --trace-summary out/*/*_kernel_trace.csv
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
SHAPES = [(1, "whisk_shuffle_124_1"), (8, "whisk_shuffle_124_8"), (64, "whisk_shuffle_124_64")]
SIDES = ("batched", "snippet")
NB = 4
FRONT_KERNELS = ("k_batch_decompress_row", "k_subgroup_row", "k_whisk_status", "k_whisk_permute_mul")


def summarize(paths):
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    print("%-22s %10s %11s %10s %8s  %-13s %s" % ("shape", "batched ms", "snippet ms", "spread ms", "ratio", "verdict", "front alone ms"))
    for _, s in SHAPES:
        med = {side: [r["shapes"][s][side + "_ms"] for r in runs] for side in SIDES}
        ys = med["snippet"]
        y, spread, f = statistics.median(ys), max(ys) - min(ys), statistics.median(med["batched"])
        verdict = "FASTER" if f < y - spread else ("slower" if f > y + spread else "no difference")
        print("%-22s %10.4f %11.4f %10.4f %7.2fx  %-13s %s   (batched runs: %s; snippet runs: %s)" %
              (s, f, y, spread, y / f, verdict, " ".join("%.4f" % r["shapes"][s]["front_ms"] for r in runs), " ".join("%.4f" % v for v in med["batched"]),
               " ".join("%.4f" % v for v in ys)))


def trace_summary(path):
    import csv

    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    short = lambda n: n.split("(")[0].split("<")[0].split("::")[-1]
    last = max(i for i, r in enumerate(rows) if "k_whisk_permute_mul" in r["Kernel_Name"])
    first = max(i for i, r in enumerate(rows[:last]) if "k_batch_decompress_row" in r["Kernel_Name"])
    while first > 0 and short(rows[first - 1]["Kernel_Name"]) in ("k_table_msm", "k_fixed_finish", "__amd_rocclr_copyBuffer"):
        first -= 1                                                       # M's two launches and the copy of their status word run ahead of the decoding
    call = rows[first: last + 1]
    t0 = int(call[0]["Start_Timestamp"])
    print("the front of the last call of %s: %d launches, %.1f us from the first kernel's start to the last one's end" %
          (os.path.basename(path), len(call), (int(call[-1]["End_Timestamp"]) - t0) / 1e3))
    print("%4s %-24s %10s %10s %10s" % ("#", "kernel", "start us", "time us", "gap us"))
    prev_end = None
    for i, r in enumerate(call):
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        print("%4d %-24s %10.1f %10.1f %10.1f" % (i, short(r["Kernel_Name"]), (s - t0) / 1e3, (e - s) / 1e3, 0.0 if prev_end is None else (s - prev_end) / 1e3))
        prev_end = e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--summarize", nargs="+")
    ap.add_argument("--target", type=int, default=0, help="five batched calls for that many shuffles (a target for rocprofv3)")
    ap.add_argument("--trace-summary")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    if a.trace_summary:
        return trace_summary(a.trace_summary)
    assert a.reps >= 30 or a.target, "the medians are taken over at least 30 repetitions"
    sys.path.insert(0, ROOT)
    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd import msm_accumulator as M
    from curdleproofs_pie_amd import prover_kernels as K
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.py_arkworks_bls12381 import CURVE_ORDER as R, G1Point, Scalar
    from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver
    from curdleproofs_pie_amd.util import random_scalar

    rng = random.Random(31)
    ell, n = 124, 124 + NB
    rs = lambda: Scalar(rng.randint(1, R - 1))
    vec = lambda m: [rs() for _ in range(m)]
    comp = lambda p: bytes(p.to_compressed_bytes())
    base = [G1Point.from_compressed_bytes(comp(p)) for p in M.batch_mul([G1Point()] * (n + 3), vec(n + 3))]
    crs = types.SimpleNamespace(vec_G=base[:ell], vec_H=base[ell:n], H=base[n], G_t=base[n + 1], G_u=base[n + 2])
    tab = FixedBaseTable(base)
    prover = ShuffleBatchProver(crs, table=tab)
    SEED = 4242

    def snippet(shuffles):
        """INTEGRATION 3k, per shuffle, from tracker bytes to post-tracker bytes and M || proof."""
        random.seed(SEED)
        provers, posts, ms = [], [], []
        for pre, perm, k, _, draws in shuffles:
            vec_R = [G1Point.from_compressed_bytes(r) for r, _ in pre]
            vec_S = [G1Point.from_compressed_bytes(s) for _, s in pre]
            vec_T, vec_U, M_, mbl = K.shuffle_permute_and_commit_input(crs, vec_R, vec_S, perm, k, table=tab)
            provers.append((crs, vec_R, vec_S, vec_T, vec_U, M_, perm, k, mbl, draws))
        proofs = K.shuffle_prove_device_many(tab, provers)
        out = []
        for pr, proof in zip(provers, proofs):
            out.append(([(comp(T), comp(U)) for T, U in zip(pr[3], pr[4])], comp(pr[5]) + proof))
        return out

    def batched(shuffles):
        return prover.prove_many(shuffles)

    out = {"reps": a.reps, "ell": ell, "shapes": {}}
    for P, name in (SHAPES if not a.target else [(a.target, "target")]):
        enc = [comp(p) for p in M.batch_mul([G1Point()] * (2 * ell * P), vec(2 * ell * P))]
        random.seed(SEED)
        shuffles = []
        for p in range(P):
            pre = list(zip(enc[2 * ell * p: 2 * ell * p + ell], enc[2 * ell * p + ell: 2 * ell * (p + 1)]))
            perm = list(range(ell))
            rng.shuffle(perm)
            mbl = [random_scalar() for _ in range(NB)]                   # what the yardstick will draw for this shuffle under the same seed
            shuffles.append((pre, perm, rs(), mbl, (vec(2), vec(NB), vec(n), vec(n - 2), *vec(5), vec(n))))
        if a.target:
            for _ in range(5):
                batched(shuffles)
            tab.close()
            return
        fns = {"batched": batched, "snippet": snippet}
        assert batched(shuffles) == snippet(shuffles), name              # the bytes are compared first
        samples = {side: [] for side in SIDES}
        for rep in range(a.reps + 2):                                    # two warm-ups, then the sides alternate
            for side in SIDES:
                t0 = time.perf_counter()
                fns[side](shuffles)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= 2:
                    samples[side].append(dt)
        # the front alone, on the same inputs
        packed = prover._pack(shuffles)
        gi, hi = prover._crs_args()[:2]
        col = lambda c: b"".join(pr[c] for pr in packed)
        front_args = (tab._tab, ell, P, gi * P, hi * P, col(0), [m for pr in packed for m in pr[1]], col(2), col(3))
        front = []
        for rep in range(a.reps + 2):
            t0 = time.perf_counter()
            tab._ctx.whisk_shuffle_front(*front_args)
            if rep >= 2:
                front.append((time.perf_counter() - t0) * 1e3)
        out["shapes"][name] = dict({side + "_ms": statistics.median(samples[side]) for side in SIDES}, front_ms=statistics.median(front))
    tab.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
