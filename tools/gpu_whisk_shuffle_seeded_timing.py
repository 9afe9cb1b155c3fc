#!/usr/bin/env python3
"""Whisk shuffles proved for a batch, from tracker bytes to post-tracker bytes and M || proof, at (ell, n_blinders) = (124, 4) for 1, 8
and 64 shuffles: the seeded face of shuffle_prover.ShuffleBatchProver (generate_packed: every draw made on the device, a status per
shuffle, csrc/capi_whisk_shuffle.h cg1_whisk_shuffle_prove_seeded) against the two faces it stands next to.

  A  random    ShuffleBatchProver.generate(lists): the permutation, k and the 3 n + 14 blinders of every shuffle drawn from Python's
               `random` and marshalled by _pack, both INSIDE the clock, then one native call
  B  seeded    ShuffleBatchProver.generate_packed(trackers96): flat bytes in and out, seed=None (32 bytes from the OS per call)
  C  given     ShuffleBatchProver.prove_many(items) with the draws made OUTSIDE the clock, as Scalars: the figure of
               profiles/r15_whisk_shuffle_prover_timing.txt
  draws        a second line, not an arm: cg1_whisk_shuffle_draws_device alone (Context.whisk_shuffle_draws_device) -- the two draw kernels,
               the copy down and the zeroing of the device buffer, with the Python conversion of the result

The three arms run in ONE process and ALTERNATE call by call; a figure is the median wall time of the Python call over --reps (>= 30)
repetitions after two warm-ups.  Before anything is timed, B under a fixed seed is compared, byte for byte, with prove_many fed
shuffle_draws_from_seed.  One run prints one JSON line.

`--summarize a.json b.json c.json` prints the table over three runs: per arm the median of the runs' medians and its spread (max - min),
B - C (the price of the device draws and the per-shuffle bookkeeping) and the verdict on B against A: FASTER / slower when the medians
differ by more than the larger of the two spreads.

    python tools/gpu_whisk_shuffle_seeded_timing.py [--reps 30] > run1.json
    python tools/gpu_whisk_shuffle_seeded_timing.py --summarize run1.json run2.json run3.json
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
ARMS = ("random", "seeded", "given")
NB = 4


def summarize(paths):
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    print("%-22s %22s %22s %22s %10s %15s  %s" % ("shape", "A random ms (spread)", "B seeded ms (spread)", "C given ms (spread)", "B - C ms", "draws alone ms", "B against A"))
    for _, s in SHAPES:
        med = {arm: [r["shapes"][s][arm + "_ms"] for r in runs] for arm in ARMS}
        m = {arm: statistics.median(v) for arm, v in med.items()}
        sp = {arm: max(v) - min(v) for arm, v in med.items()}
        spread = max(sp["random"], sp["seeded"])
        verdict = "FASTER" if m["seeded"] < m["random"] - spread else ("slower" if m["seeded"] > m["random"] + spread else "no difference")
        cell = lambda arm: "%10.4f (%8.4f)" % (m[arm], sp[arm])
        print("%-22s %22s %22s %22s %10.4f %15.4f  %-13s (%s)" % (s, cell("random"), cell("seeded"), cell("given"), m["seeded"] - m["given"],
                                                                 statistics.median(r["shapes"][s]["draws_ms"] for r in runs), verdict,
                                                          "; ".join("%s runs: %s" % (arm, " ".join("%.4f" % v for v in med[arm])) for arm in ARMS)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--summarize", nargs="+")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    assert a.reps >= 30, "the medians are taken over at least 30 repetitions"
    sys.path.insert(0, ROOT)
    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd import msm_accumulator as M
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.py_arkworks_bls12381 import CURVE_ORDER as R, G1Point, Scalar
    from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver, shuffle_draws_from_seed

    rng = random.Random(31)
    ell, n = 124, 124 + NB
    rs = lambda: Scalar(rng.randint(1, R - 1))
    vec = lambda m: [rs() for _ in range(m)]
    comp = lambda p: bytes(p.to_compressed_bytes())
    base = [G1Point.from_compressed_bytes(comp(p)) for p in M.batch_mul([G1Point()] * (n + 3), vec(n + 3))]
    crs = types.SimpleNamespace(vec_G=base[:ell], vec_H=base[ell:n], H=base[n], G_t=base[n + 1], G_u=base[n + 2])
    tab = FixedBaseTable(base)
    prover = ShuffleBatchProver(crs, table=tab)
    seed = bytes(range(32))

    out = {"reps": a.reps, "ell": ell, "shapes": {}}
    for P, name in SHAPES:
        enc = [comp(p) for p in M.batch_mul([G1Point()] * (2 * ell * P), vec(2 * ell * P))]
        lists = [list(zip(enc[2 * ell * p: 2 * ell * p + ell], enc[2 * ell * p + ell: 2 * ell * (p + 1)])) for p in range(P)]
        trackers96 = b"".join(r + s for pre in lists for r, s in pre)
        items = []
        for pre in lists:
            perm = list(range(ell))
            rng.shuffle(perm)
            items.append((pre, perm, rs(), vec(NB), (vec(2), vec(NB), vec(n), vec(n - 2), *vec(5), vec(n))))
        # the bytes first: the seeded call against its definition
        post, proofs, status = prover.generate_packed(trackers96, seed=seed)
        want = prover.prove_many([(pre, *shuffle_draws_from_seed(seed, i, ell)) for i, pre in enumerate(lists)])
        assert status == [0] * P and proofs == b"".join(pf for _, pf in want) and post == b"".join(r + s for tr, _ in want for r, s in tr), name
        fns = {"random": lambda: prover.generate(lists), "seeded": lambda: prover.generate_packed(trackers96), "given": lambda: prover.prove_many(items)}
        samples = {arm: [] for arm in ARMS}
        for rep in range(a.reps + 2):                                    # two warm-ups, then the arms alternate
            for arm in ARMS:
                t0 = time.perf_counter()
                fns[arm]()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= 2:
                    samples[arm].append(dt)
        draws = []
        for rep in range(a.reps + 2):
            t0 = time.perf_counter()
            tab._ctx.whisk_shuffle_draws_device(ell, P, seed, 0)
            if rep >= 2:
                draws.append((time.perf_counter() - t0) * 1e3)
        out["shapes"][name] = dict({arm + "_ms": statistics.median(samples[arm]) for arm in ARMS}, draws_ms=statistics.median(draws))
    tab.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
