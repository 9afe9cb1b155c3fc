#!/usr/bin/env python3
"""What a batch costs when some of its proofs carry a point outside G1, for both batch verifiers.

  shuffle arm   ShuffleBatchVerifier.verify_packed over 1 024 proofs at ell = 124 (tests/golden/shuffle_batch_ell124*), of which 0, 1, 4, 16, 64 or
                all 1 024 are replaced by the flagged proof the reference ACCEPTS of tests/golden/exact_device_vectors.json ("ell124": cancelling
                torsion over the same CRS)
  opening arm   OpeningBatchVerifier.verify_packed over 65 536 proofs of which 0, 1, 16, 256 or all 65 536 are the flagged-and-accepted proof of
                tests/golden/torsion_vectors.json ("k_G + T3, A + c*T3"), the rest its honest one
An accepted flagged proof, because a rejected one leaves the per-proof path at its first failing equality and flatters it.

  A  host     exact_device=False: every flagged proof decided on its own (_decide_flagged / cg1_opening_exact: the path before the device pass
              existed; on a checkout without the keyword the verifiers are built without it)
  B  device   exact_device=True: all flagged proofs of the batch in one device pass (k_exact_relations)

The arms run in ONE process and ALTERNATE call by call; a figure is the median wall time of the call over --reps (>= 30) repetitions after
one warm-up -- except where the warm-up call of an arm took more than --slow-ms (default 2 000): that arm then runs 3 repetitions at that
count, and the line says so.  Verdicts are compared between the arms before anything is timed.
One run prints one JSON line; `--summarize a.json b.json c.json` prints a table per arm over three runs: per arm the median of the runs' medians
and its spread (max - min), and B against A: FASTER / slower when the medians differ by more than the larger of the two spreads.
EXACT_DEVICE_MIN of a verifier is the smallest flagged count from which B is FASTER.

    python tools/gpu_exact_device_timing.py [--reps 30] [--only shuffle|opening] > run1.json
    python tools/gpu_exact_device_timing.py --summarize run1.json run2.json run3.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("host", "device")
WORKLOADS = {"shuffle": (1024, (0, 1, 4, 16, 64, 1024)), "opening": (65536, (0, 1, 16, 256, 65536))}


def summarize(paths):
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    for kind, (n, counts) in WORKLOADS.items():
        if not all(kind in r for r in runs):
            continue
        print("%s proofs: %d per batch; median wall ms of verify_packed (spread over %d runs)" % (kind, n, len(runs)))
        print("%8s %24s %24s %9s  %s" % ("flagged", "A host ms (spread)", "B device ms (spread)", "A / B", "B against A"))
        for f in counts:
            med = {arm: [r[kind][str(f)][arm + "_ms"] for r in runs] for arm in ARMS}
            m = {arm: statistics.median(v) for arm, v in med.items()}
            sp = {arm: max(v) - min(v) for arm, v in med.items()}
            spread = max(sp.values())
            verdict = "FASTER" if m["device"] < m["host"] - spread else ("slower" if m["device"] > m["host"] + spread else "no difference")
            reps = "reps " + " / ".join(str(runs[0][kind][str(f)][arm + "_reps"]) for arm in ARMS)
            cell = lambda arm: "%12.3f (%9.3f)" % (m[arm], sp[arm])
            print("%8d %24s %24s %9.2f  %-13s (%s; %s)" % (f, cell("host"), cell("device"), m["host"] / m["device"], verdict, reps,
                                                          "; ".join("%s runs: %s" % (arm, " ".join("%.3f" % v for v in med[arm])) for arm in ARMS)))
        print()


def run_arms(a, n, counts, make_batch, calls, paths):
    """calls[arm](batch) -> verdict list; paths[arm]() -> the path the last call took (None where the checkout does not say)"""
    res = {}
    for f in counts:
        step = n // f if f else 0                           # the flagged proofs spread evenly through the batch
        which = [bool(f) and i % step == 0 for i in range(n)]
        assert sum(which) == f
        batch = make_batch(which)
        samples, reps = {arm: [] for arm in ARMS}, {}
        for arm in ARMS:                                    # the warm-up: the verdicts, and how long a call of this arm takes here
            t0 = time.perf_counter()
            assert calls[arm](batch) == [True] * n, (f, arm)
            reps[arm] = a.reps if (time.perf_counter() - t0) * 1e3 <= a.slow_ms else 3
            got = paths[arm]()
            assert got in ("n/a", arm if f else None), (f, arm, got)
        for rep in range(max(reps.values())):               # the arms alternate
            for arm in ARMS:
                if rep < reps[arm]:
                    t0 = time.perf_counter()
                    calls[arm](batch)
                    samples[arm].append((time.perf_counter() - t0) * 1e3)
        res[str(f)] = dict({arm + "_ms": statistics.median(samples[arm]) for arm in ARMS}, **{arm + "_reps": reps[arm] for arm in ARMS})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--slow-ms", type=float, default=2000.0)
    ap.add_argument("--only", choices=tuple(WORKLOADS))
    ap.add_argument("--summarize", nargs="+")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    assert a.reps >= 30, "the medians are taken over at least 30 repetitions"
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd.shuffle_verifier import OpeningBatchVerifier, ShuffleBatchVerifier

    def pair(make):
        try:
            return {"host": make(exact_device=False), "device": make(exact_device=True)}
        except TypeError:                                  # a checkout from before the keyword: both arms are the per-proof path
            return {"host": make(), "device": make()}

    out = {"reps": a.reps}
    if a.only in (None, "shuffle"):
        from batch_fixture import ShuffleBatch

        fx = ShuffleBatch()
        n, counts = WORKLOADS["shuffle"]
        assert fx.count >= n and fx.ell == 124
        c = json.load(open(os.path.join(ROOT, "tests", "golden", "exact_device_vectors.json")))["ell124"]
        assert c["accepts"]
        f_inst, f_proof = bytes.fromhex(c["pre_r"] + c["pre_k"] + c["post_r"] + c["post_k"]), bytes.fromhex(c["proof"])
        vs = pair(lambda **kw: ShuffleBatchVerifier(fx.crs, N.Context(0), **kw))
        make_batch = lambda which: (b"".join(f_inst if w else fx.instances[i] for i, w in enumerate(which)),
                                    b"".join(f_proof if w else fx.proofs[i] for i, w in enumerate(which)))
        calls = {arm: (lambda batch, v=vs[arm]: [s == 0 for s in v.verify_packed(batch[0], batch[1], n)]) for arm in ARMS}
        paths = {arm: (lambda v=vs[arm]: v.last_stats.get("exact_path", "n/a")) for arm in ARMS}
        out["shuffle"] = run_arms(a, n, counts, make_batch, calls, paths)
        for v in vs.values():
            v.close()
    if a.only in (None, "opening"):
        t = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_vectors.json")))["opening"]
        wire = lambda c: (bytes.fromhex(c["r_G"] + c["k_r_G"]), bytes.fromhex(c["k_commitment"]), bytes.fromhex(c["proof"]))
        honest = wire(next(c for c in t if c["name"] == "honest"))
        flagged = wire(next(c for c in t if c["name"].startswith("k_G + T3") and c["accepts"]))
        n, counts = WORKLOADS["opening"]
        ctx = N.Context(0)
        vs = pair(lambda **kw: OpeningBatchVerifier(ctx, **kw))
        make_batch = lambda which: tuple(b"".join((flagged if w else honest)[k] for w in which) for k in range(3))
        calls = {arm: (lambda batch, v=vs[arm]: v.verify_packed(*batch)) for arm in ARMS}
        paths = {arm: (lambda v=vs[arm]: getattr(v, "last_exact_path", "n/a")) for arm in ARMS}
        out["opening"] = run_arms(a, n, counts, make_batch, calls, paths)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
