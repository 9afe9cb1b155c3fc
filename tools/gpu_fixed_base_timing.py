#!/usr/bin/env python3
"""Fixed-base tables (curdleproofs_pie_amd/fixed_base.py, csrc/kernels_fixed.h) against the paths they would replace, pair by pair in
ONE process on one GPU: the median of --reps (>= 20) repetitions after a warm-up, both sides printed.

  shape                                          fixed-base side        yardstick
  one IPA round: 4 MSMs x 65 terms               tab.msm_many           compute_MSM_batch on the same terms
  the same for 8 / 64 provers in step (32 / 256) tab.msm_many           compute_MSM_batch
  single MSM of 128 / 133 terms                  tab.msm                compute_MSM (forced)
  ipa_rounds at n = 128, one prover, wall        table=                 no table
  ipa_rounds_many at n = 128, eight provers      table=                 no table
  table build time and nbytes for 133 bases      reported               --

`--shapes` instead times the launch shapes of k_table_msm against each other on the IPA-round calls ("fixed_waves" x "fixed_slice"
through cg1_ctx_set_param; 0 / 0 = the library's own choice): the measurement behind the rule in csrc/capi_fixed.h.

One run prints one JSON line.  `--summarize a.json b.json c.json` reads three runs and prints the table with the verdict per shape:
the fixed-base path counts as FASTER when its median (the median of the runs) lies below the yardstick's by more than the spread
(max - min) between the yardstick's own medians over the runs.

    python tools/gpu_fixed_base_timing.py [--reps 30] > run1.json
    python tools/gpu_fixed_base_timing.py --summarize run1.json run2.json run3.json
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["ipa_round_4x65", "ipa_round_8_provers_32x65", "ipa_round_64_provers_256x65", "single_128", "single_133", "ipa_rounds_n128_1_prover",
          "ipa_rounds_many_n128_8_provers"]


def median_ms(fn, reps):
    fn(); fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def summarize(paths):
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    print("%-34s %12s %12s %10s %10s  %s" % ("shape", "fixed ms", "yardstick ms", "spread ms", "ratio", "verdict"))
    for s in SHAPES:
        fx = [r["shapes"][s]["fixed_ms"] for r in runs]
        ys = [r["shapes"][s]["yardstick_ms"] for r in runs]
        f, y, spread = statistics.median(fx), statistics.median(ys), max(ys) - min(ys)
        verdict = "FASTER" if f < y - spread else ("slower" if f > y + spread else "no difference")
        print("%-34s %12.4f %12.4f %10.4f %9.2fx  %s   (fixed runs: %s; yardstick runs: %s)" %
              (s, f, y, spread, y / f, verdict, " ".join("%.4f" % v for v in fx), " ".join("%.4f" % v for v in ys)))
    print("table of 133 bases: build %s ms, %d bytes (%.1f MiB)" % (" ".join("%.1f" % r["table_133"]["build_ms"] for r in runs), runs[0]["table_133"]["nbytes"],
                                                                     runs[0]["table_133"]["nbytes"] / 2 ** 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--summarize", nargs="+")
    ap.add_argument("--shapes", action="store_true", help="A/B of k_table_msm's launch shapes on the IPA-round calls")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    assert a.reps >= 20, "the medians are taken over at least 20 repetitions"
    sys.path.insert(0, ROOT)
    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd import msm_accumulator as M
    from curdleproofs_pie_amd import prover_kernels as K
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.py_arkworks_bls12381 import CURVE_ORDER as R, G1Point, Scalar

    rng = random.Random(11)
    rs = lambda: Scalar(rng.randint(1, R - 1))
    pts = lambda m: M.batch_mul([G1Point()] * m, [rs() for _ in range(m)])
    out = {"reps": a.reps, "shapes": {}}

    crs = pts(133)                                               # an ell = 124 CRS: vec_G | vec_H | H | G_t | G_u | G_sum | H_sum
    M.points_to_affine96(crs)
    t = time.perf_counter()
    tab = FixedBaseTable(crs)
    out["table_133"] = {"build_ms": (time.perf_counter() - t) * 1e3, "nbytes": tab.nbytes}

    def pair(name, fixed, yard):
        out["shapes"][name] = {"fixed_ms": median_ms(fixed, a.reps), "yardstick_ms": median_ms(yard, a.reps)}

    # the four MSMs of a halving round at n = 128: 64 bases (+ H for the two C-side sums), for 1 / 8 / 64 provers in step
    G, Gp, H = crs[:128], crs[:128][::-1], crs[128]
    for provers, name in ((1, "ipa_round_4x65"), (8, "ipa_round_8_provers_32x65"), (64, "ipa_round_64_provers_256x65")):
        jobs = []
        for _ in range(provers):
            for half, with_h in ((G[64:], True), (Gp[:64], True), (G[:64], True), (Gp[64:], True)):
                bases = list(half) + ([H] if with_h else [])
                jobs.append((bases, [rs() for _ in bases]))
        assert all(len(b) == 65 for b, _ in jobs)
        if a.shapes:
            ctx, res = N.default_context(), {}
            for waves in (0, 4, 8, 16):
                for sl in ((0,) if waves == 0 else (1, 2, 4, 8, 16, 32)):
                    ctx.set_param("fixed_waves", waves); ctx.set_param("fixed_slice", sl)
                    res["waves %d slice %d" % (waves, sl)] = round(median_ms(lambda: tab.msm_many(jobs), a.reps), 4)
            ctx.set_param("fixed_waves", 0); ctx.set_param("fixed_slice", 0)
            out["shapes"][name] = res
            continue
        pair(name, lambda: tab.msm_many(jobs), lambda: M.compute_MSM_batch(jobs))
    if a.shapes:
        tab.close()
        print(json.dumps(out))
        return
    for n in (128, 133):
        sc = [rs() for _ in range(n)]
        bases = crs[:n]
        pair("single_%d" % n, lambda: tab.msm(sc, bases), lambda: M.compute_MSM(bases, sc)._b)

    # whole halving loops (7 rounds at n = 128), wall time with the Python marshalling; fixed challenges (the transcript is the caller's)
    Gv, Gpv = pts(128), pts(128)
    Hh = pts(1)[0]
    tab.close()
    tab2 = FixedBaseTable(Gv + Gpv + [Hh])
    gam = [rs() for _ in range(8)]
    const = lambda: (lambda g: (lambda *p: g.pop(0)))(list(gam))
    c, d = [rs() for _ in range(128)], [rs() for _ in range(128)]
    pair("ipa_rounds_n128_1_prover", lambda: K.ipa_rounds(Gv, Gpv, Hh, c, d, const(), table=tab2), lambda: K.ipa_rounds(Gv, Gpv, Hh, c, d, const()))
    rot = lambda v, k: v[k:] + v[:k]
    provers = [(Gv, Gpv, Hh, rot(c, k), rot(d, k)) for k in range(8)]
    pair("ipa_rounds_many_n128_8_provers", lambda: K.ipa_rounds_many(provers, [const() for _ in provers], table=tab2),
         lambda: K.ipa_rounds_many(provers, [const() for _ in provers]))
    tab2.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
