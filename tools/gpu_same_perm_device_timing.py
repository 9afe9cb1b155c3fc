#!/usr/bin/env python3
"""The same-permutation argument proved on the device (prover_kernels.same_permutation_prove_device_many, csrc/kernels_same_perm.h) against
the best path without it, at (ell, n_blinders) = (124, 4) for 1, 8 and 64 provers in step: the whole of SamePermutationProof.new
(same_perm.py:27-72) after its callee's draws, inputs as Python objects in, proof bytes out.

  device     same_permutation_prove_device_many: the transcript head on the host inside the C entry, one launch chain, one wait
  yardstick  the wrapper's head on the host -- the host transcript, the polynomial factors and their product in Python ints, the B's by
             one table.msm_many -- followed by grand_product_prove_device_many (one launch chain): two waits

Both run in ONE process and ALTERNATE call by call; the figure is the median wall time of the Python call over --reps (>= 30)
repetitions after two warm-ups.  Fresh transcripts are made outside the timed region.  Both sides must produce the same bytes and the
same transcript states (checked once per shape).  One run prints one JSON line; it also carries, per shape, the C entry alone and what
lane 0 of the step kernels (k_gprod_step and k_ipa_step together) reports in shader-clock ticks.

`--summarize a.json b.json c.json` prints the table over three runs: a shape counts as FASTER when the device median (the median of
the runs) lies below the yardstick's by more than the spread (max - min) of the yardstick's own medians.

`--target P` is a short target for `rocprofv3 --kernel-trace --stats`: five device calls for P provers and nothing else;
`--trace-summary kernel_trace.csv` then prints, for the LAST chain of the trace, every kernel's time and the gap before it.

    python tools/gpu_same_perm_device_timing.py [--reps 30] > run1.json
    python tools/gpu_same_perm_device_timing.py --summarize run1.json run2.json run3.json
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/gpu_same_perm_device_timing.py --target 8
    python tools/gpu_same_perm_device_timing.py --trace-summary out/*/*_kernel_trace.csv
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, "same_perm_new_124_4_1_prover"), (8, "same_perm_new_124_4_8_provers"), (64, "same_perm_new_124_4_64_provers")]


def summarize(paths):
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    print("%-32s %12s %12s %10s %10s  %s" % ("shape", "device ms", "yardstick ms", "spread ms", "ratio", "verdict"))
    for _, s in SHAPES:
        dv = [r["shapes"][s]["device_ms"] for r in runs]
        ys = [r["shapes"][s]["yardstick_ms"] for r in runs]
        f, y, spread = statistics.median(dv), statistics.median(ys), max(ys) - min(ys)
        verdict = "FASTER" if f < y - spread else ("slower" if f > y + spread else "no difference")
        print("%-32s %12.4f %12.4f %10.4f %9.2fx  %s   (device runs: %s; yardstick runs: %s)" %
              (s, f, y, spread, y / f, verdict, " ".join("%.4f" % v for v in dv), " ".join("%.4f" % v for v in ys)))
    for _, s in SHAPES:
        r = runs[0]["shapes"][s]
        print("%-32s C entry alone %.4f ms; lane 0, ticks per prover: %s" % (s, r["c_entry_ms"], json.dumps(r["lane0_ticks"])))


def trace_summary(path):
    import csv

    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    short = lambda n: n.split("(")[0].split("::")[-1].split("<")[0]
    begins = [i for i, r in enumerate(rows) if "k_same_perm_begin" in r["Kernel_Name"]]
    chain = rows[begins[-1]:]
    last = max(i for i, r in enumerate(chain) if "k_ipa_step" in r["Kernel_Name"])
    chain = chain[: last + 1]
    t0 = int(chain[0]["Start_Timestamp"])
    print("the last chain of %s: %d launches, %.1f us from the first kernel's start to the last one's end" %
          (os.path.basename(path), len(chain), (int(chain[-1]["End_Timestamp"]) - t0) / 1e3))
    print("%4s %-18s %10s %10s %10s" % ("#", "kernel", "start us", "time us", "gap us"))
    tot, prev_end = {}, None
    for i, r in enumerate(chain):
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        gap = 0.0 if prev_end is None else (s - prev_end) / 1e3
        print("%4d %-18s %10.1f %10.1f %10.1f" % (i, short(r["Kernel_Name"]), (s - t0) / 1e3, (e - s) / 1e3, gap))
        k = tot.setdefault(short(r["Kernel_Name"]), [0, 0.0])
        k[0] += 1; k[1] += (e - s) / 1e3
        tot.setdefault("(gaps)", [0, 0.0])[1] += gap
        prev_end = e
    for name, (cnt, us) in tot.items():
        print("%-18s %3d launches %10.1f us" % (name, cnt, us))


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
    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd import msm_accumulator as M
    from curdleproofs_pie_amd import prover_kernels as K
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.py_arkworks_bls12381 import CURVE_ORDER as R, G1Point, Scalar

    rng = random.Random(22)
    ell, nb = 124, 4
    n = ell + nb
    rs = lambda: Scalar(rng.randint(1, R - 1))
    vec = lambda m: [rs() for _ in range(m)]
    bases = M.batch_mul([G1Point()] * (n + 1), vec(n + 1))
    M.points_to_affine96(bases)
    tab = FixedBaseTable(bases)
    vec_G, U = list(range(n)), n
    ctx = N.default_context()
    comp = lambda p: bytes(p.to_compressed_bytes())
    fr32 = lambda s: bytes(s.to_le_bytes())
    sc = lambda v: [Scalar(x) for x in v]

    def proof_bytes(B, gp):
        C, r_p, (B_c, B_d, LC, RC, LD, RD, c_fin, d_fin) = gp
        return comp(B) + comp(C) + fr32(r_p) + b"".join(comp(p) for p in [B_c, B_d] + list(LC) + list(RC) + list(LD) + list(RD)) + fr32(c_fin) + fr32(d_fin)

    def host_driven(provers, ts):
        """SamePermutationProof.new after its callee's draws for provers in step: the wrapper on the host, then the grand-product chain."""
        heads = []
        for (_, _, _, A, Mc, va, perm, abl, mbl, cbl, r, zh), t in zip(provers, ts):
            t.append_list(b"same_perm_step1", [comp(A), comp(Mc)])
            t.append_list(b"same_perm_step1", [fr32(x) for x in va])
            alpha = int(t.get_and_append_challenge(b"same_perm_alpha"))
            beta = int(t.get_and_append_challenge(b"same_perm_beta"))
            ai = [int(x) for x in va]
            b = [(ai[m] + m * alpha + beta) % R for m in perm]
            prod = 1
            for x in b:
                prod = prod * x % R
            heads.append((sc(b), sc((int(x) + alpha * int(y)) % R for x, y in zip(abl, mbl)), Scalar(prod)))
        Bs = tab.msm_many([(vec_G, h[0] + h[1]) for h in heads])
        gps = K.grand_product_prove_device_many(tab, [(pr[0], pr[1], pr[2], B, h[2], h[0], h[1], pr[9], pr[10], pr[11]) for pr, h, B in zip(provers, heads, Bs)], ts)
        return [proof_bytes(B, gp) for B, gp in zip(Bs, gps)]

    def device(provers, ts):
        return [proof_bytes(*res) for res in K.same_permutation_prove_device_many(tab, provers, ts)]

    out = {"reps": a.reps, "ell": ell, "n_blinders": nb, "shapes": {}}
    for P, name in (SHAPES if not a.target else [(a.target, "target")]):
        provers = []
        for _ in range(P):
            va, perm, abl, mbl = vec(ell), rng.sample(range(ell), ell), vec(nb - 2) + [Scalar(0), Scalar(0)], vec(nb)      # curdleproofs.py:73-74
            A = tab.msm([va[m] for m in perm] + abl, vec_G)
            Mc = tab.msm([Scalar(m) for m in perm] + mbl, vec_G)
            provers.append((vec_G[:ell], vec_G[ell:], U, A, Mc, va, perm, abl, mbl, vec(nb), vec(n), vec(n - 2)))
        M.points_to_affine96([x for pr in provers for x in pr[3:5]])     # normalised once, outside the timed region, for both sides
        mk = lambda: [CurdleproofsTranscript(b"timing %d" % p) for p in range(P)]
        t1, t2 = mk(), mk()
        assert device(provers, t1) == host_driven(provers, t2), name
        assert [bytes(t.strobe._st.raw) for t in t1] == [bytes(t.strobe._st.raw) for t in t2], name
        if a.target:
            for _ in range(5):
                device(provers, mk())
            tab.close()
            return
        samples = {"device": [], "yardstick": []}
        for rep in range(a.reps + 2):                                    # two warm-ups, then the two paths alternate
            for side, fn in (("device", device), ("yardstick", host_driven)):
                ts = mk()
                t0 = time.perf_counter()
                fn(provers, ts)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= 2:
                    samples[side].append(dt)
        rec = {"device_ms": statistics.median(samples["device"]), "yardstick_ms": statistics.median(samples["yardstick"])}
        # the C entry alone (arguments already packed), and what lane 0 reports
        flat = lambda k: b"".join(fr32(s) for pr in provers for s in pr[k])
        args = (list(range(n)) * P, [U] * P, b"".join(comp(x) for pr in provers for x in pr[3:5]), flat(5), [m for pr in provers for m in pr[6]], flat(7), flat(8),
                flat(9), flat(10), flat(11))
        entry = []
        with tab._ctx_lock():
            for rep in range(a.reps + 2):
                states = b"".join(bytes(t.strobe._st.raw) for t in mk())
                t0 = time.perf_counter()
                _, _, ck = ctx.same_perm_prove_device(tab._tab, ell, nb, P, *args, states, want_clocks=True)
                if rep >= 2:
                    entry.append((time.perf_counter() - t0) * 1e3)
        rec["c_entry_ms"] = statistics.median(entry)
        mean = lambda k: round(statistics.mean(ck[4 * p + k] for p in range(P)), 1)
        rec["lane0_ticks"] = {"transcript_steps": ck[3], "transcript": mean(0), "inversions": mean(1), "steps_that_emit_terms": mean(2)}
        out["shapes"][name] = rec
    tab.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
