#!/usr/bin/env python3
"""Seeded Whisk shuffles with the witness resident on the device against the copying path, and the copying path against the commit before
it: ShuffleBatchProver.generate_packed (cg1_whisk_shuffle_prove_seeded, csrc/capi_whisk_shuffle.h) at ell = 124 for 1, 8 and 64 shuffles,
tracker bytes to post-tracker bytes and M || proof, seed=None.

  parent    a build of the parent commit: its own tree (--root), its own library
  off       this commit, "whisk_resident_witness" = 0: the path the parent runs, which must not pay for the new one
  on        this commit, "whisk_resident_witness" = 1: no copy of the draws down, k_whisk_witness_place instead of the host staging

Every arm is a process of its own (one `--arm` run prints one JSON line: per shape the median wall time of the Python call over --reps
repetitions after two warm-ups).  `--rounds` runs the three arms one after the other, three times over, each child under its own
`timeout`, and stops at the first child that fails; `--summarize` prints the table over the lines it wrote: per arm the median of the
rounds' medians with min .. max, whether `off` lies within `parent`'s own min .. max at every shape (the one condition), and `on`
against `off` as measured.

    python tools/gpu_whisk_resident_timing.py --rounds OUT_DIR --parent-root PARENT_TREE [--reps 30]
    python tools/gpu_whisk_resident_timing.py --summarize OUT_DIR
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, "whisk_shuffle_124_1"), (8, "whisk_shuffle_124_8"), (64, "whisk_shuffle_124_64")]
ARMS = ("parent", "off", "on")
ROUNDS = 3
NB = 4
ARM_TIMEOUT_S = 170


def run_arm(arm, root, reps):
    sys.path.insert(0, root)
    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd import msm_accumulator as M
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.py_arkworks_bls12381 import CURVE_ORDER as R, G1Point, Scalar
    from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver

    rng = random.Random(31)
    ell, n = 124, 124 + NB
    vec = lambda m: [Scalar(rng.randint(1, R - 1)) for _ in range(m)]
    comp = lambda p: bytes(p.to_compressed_bytes())
    base = [G1Point.from_compressed_bytes(comp(p)) for p in M.batch_mul([G1Point()] * (n + 3), vec(n + 3))]
    crs = types.SimpleNamespace(vec_G=base[:ell], vec_H=base[ell:n], H=base[n], G_t=base[n + 1], G_u=base[n + 2])
    tab = FixedBaseTable(base)
    prover = ShuffleBatchProver(crs, table=tab) if arm != "on" else ShuffleBatchProver(crs, table=tab, resident_witness=True)
    out = {"arm": arm, "reps": reps, "ell": ell, "shapes": {}}
    for P, name in SHAPES:
        enc = [comp(p) for p in M.batch_mul([G1Point()] * (2 * ell * P), vec(2 * ell * P))]
        trackers96 = b"".join(enc[2 * ell * p + i] + enc[2 * ell * p + ell + i] for p in range(P) for i in range(ell))
        post, proofs, status = prover.generate_packed(trackers96, seed=bytes(range(32)))
        assert status == [0] * P
        out["shapes"][name + "_sha"] = __import__("hashlib").sha256(post + proofs).hexdigest()[:16]       # the arms prove the same bytes
        samples = []
        for rep in range(reps + 2):
            t0 = time.perf_counter()
            prover.generate_packed(trackers96)
            if rep >= 2:
                samples.append((time.perf_counter() - t0) * 1e3)
        out["shapes"][name] = statistics.median(samples)
    tab.close()
    print(json.dumps(out))


def rounds(out_dir, parent_root, reps):
    os.makedirs(out_dir, exist_ok=True)
    for r in range(ROUNDS):
        for arm in ARMS:
            root = parent_root if arm == "parent" else ROOT
            cmd = ["timeout", "-k", "10", str(ARM_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--arm", arm, "--root", root, "--reps", str(reps)]
            done = subprocess.run(cmd, capture_output=True, text=True)
            if done.returncode != 0:
                sys.stderr.write(done.stdout + done.stderr)
                sys.exit("arm %s of round %d ended with status %d: nothing more is started" % (arm, r, done.returncode))
            with open(os.path.join(out_dir, "round%d_%s.json" % (r, arm)), "w") as f:
                f.write(done.stdout.strip().splitlines()[-1] + "\n")
            print("round %d %-6s %s" % (r, arm, done.stdout.strip().splitlines()[-1]), flush=True)


def summarize(out_dir):
    runs = {arm: [json.load(open(os.path.join(out_dir, "round%d_%s.json" % (r, arm)))) for r in range(ROUNDS)] for arm in ARMS}
    print("%-22s %30s %30s %30s  %-28s %s" % ("shape", "parent ms (min .. max)", "off ms (min .. max)", "on ms (min .. max)", "off within parent's spread", "on against off"))
    ok = True
    for _, s in SHAPES:
        v = {arm: [r["shapes"][s] for r in runs[arm]] for arm in ARMS}
        assert len({r["shapes"][s + "_sha"] for arm in ARMS for r in runs[arm]}) == 1, "the arms proved different bytes"
        m = {arm: statistics.median(x) for arm, x in v.items()}
        cell = lambda arm: "%9.3f (%8.3f .. %8.3f)" % (m[arm], min(v[arm]), max(v[arm]))
        within = min(v["parent"]) <= m["off"] <= max(v["parent"])
        ok = ok and within
        print("%-22s %30s %30s %30s  %-28s %+.3f ms (%+.1f %%)" % (s, cell("parent"), cell("off"), cell("on"), "yes" if within else "NO", m["on"] - m["off"],
                                                                  100.0 * (m["on"] - m["off"]) / m["off"]))
    print("condition (off within parent's min .. max at every shape): %s" % ("holds" if ok else "DOES NOT HOLD"))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--rounds", metavar="OUT_DIR")
    ap.add_argument("--parent-root")
    ap.add_argument("--summarize", metavar="OUT_DIR")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    if a.rounds:
        assert a.parent_root, "--rounds needs --parent-root: a tree of the parent commit with its library built"
        return rounds(a.rounds, os.path.abspath(a.parent_root), a.reps)
    assert a.arm, "one of --arm, --rounds, --summarize"
    return run_arm(a.arm, os.path.abspath(a.root), a.reps)


if __name__ == "__main__":
    sys.exit(main())
