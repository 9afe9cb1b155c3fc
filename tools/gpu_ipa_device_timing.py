#!/usr/bin/env python3
"""The inner-product argument proved on the device (prover_kernels.ipa_prove_device_many, csrc/kernels_ipa.h) against the host-driven
path it would replace, at n = 128 for 1, 8 and 64 provers in step: the whole of IPA.new (ipa.py:97-153) after the blinder draw, inputs as
Python objects in, proof bytes out.

  device     ipa_prove_device_many: one launch chain, one wait
  yardstick  the host-driven path: table.msm_many for B_c / B_d, the host transcript, ipa_rounds_many(..., table=), the points compressed

Both run in ONE process and ALTERNATE call by call; the figure is the median wall time of the Python call over --reps (>= 30)
repetitions after two warm-ups.  Fresh transcripts are made outside the timed region.  Both sides must produce the same bytes (checked
once per shape).  One run prints one JSON line; it also carries, per shape, what lane 0 of k_ipa_step reports about its serial part
(shader-clock ticks in the transcript and in the inversion of gamma, per step), for both inversions ("ipa_inv" 0 / 1).

`--summarize a.json b.json c.json` prints the table over three runs: a shape counts as FASTER when the device median (the median of
the runs) lies below the yardstick's by more than the spread (max - min) of the yardstick's own medians.

`--target P` is a short target for `rocprofv3 --kernel-trace --stats`: five device calls for P provers and nothing else;
`--trace-summary kernel_trace.csv` then prints, for the LAST chain of the trace, every kernel's time and the gap before it.

    python tools/gpu_ipa_device_timing.py [--reps 30] > run1.json
    python tools/gpu_ipa_device_timing.py --summarize run1.json run2.json run3.json
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/gpu_ipa_device_timing.py --target 8
    python tools/gpu_ipa_device_timing.py --trace-summary out/*/*_kernel_trace.csv
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, "ipa_new_n128_1_prover"), (8, "ipa_new_n128_8_provers"), (64, "ipa_new_n128_64_provers")]


def summarize(paths):
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    print("%-28s %12s %12s %10s %10s  %s" % ("shape", "device ms", "yardstick ms", "spread ms", "ratio", "verdict"))
    for _, s in SHAPES:
        dv = [r["shapes"][s]["device_ms"] for r in runs]
        ys = [r["shapes"][s]["yardstick_ms"] for r in runs]
        f, y, spread = statistics.median(dv), statistics.median(ys), max(ys) - min(ys)
        verdict = "FASTER" if f < y - spread else ("slower" if f > y + spread else "no difference")
        print("%-28s %12.4f %12.4f %10.4f %9.2fx  %s   (device runs: %s; yardstick runs: %s)" %
              (s, f, y, spread, y / f, verdict, " ".join("%.4f" % v for v in dv), " ".join("%.4f" % v for v in ys)))
    for _, s in SHAPES:
        for r in runs[:1]:
            print("%-28s device with a^(r-2) instead of the binary inversion: %.4f ms;  lane 0 per step, ticks: %s" %
                  (s, r["shapes"][s]["device_fermat_ms"], json.dumps(r["shapes"][s]["lane0_ticks"])))


def trace_summary(path):
    import csv

    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    short = lambda n: n.split("(")[0].split("::")[-1]
    begins = [i for i, r in enumerate(rows) if "k_ipa_step" in r["Kernel_Name"] and (i == 0 or "k_fixed_finish" not in rows[i - 1]["Kernel_Name"])]
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

    rng = random.Random(17)
    n = 128
    rs = lambda: Scalar(rng.randint(1, R - 1))
    vec = lambda: [rs() for _ in range(n)]
    pts = M.batch_mul([G1Point()] * (2 * n + 1), [rs() for _ in range(2 * n + 1)])
    M.points_to_affine96(pts)
    G, Gp, H = pts[:n], pts[n:2 * n], pts[2 * n]
    tab = FixedBaseTable(pts)
    ctx = N.default_context()
    comp = lambda ps: [bytes(p.to_compressed_bytes()) for p in ps]
    fr32 = lambda s: bytes(s.to_le_bytes())

    def proof_bytes(B_c, B_d, LC, RC, LD, RD, c_fin, d_fin):
        return b"".join(comp([B_c, B_d] + list(LC) + list(RC) + list(LD) + list(RD))) + fr32(c_fin) + fr32(d_fin)

    def host_driven(provers, ts):
        """IPA.new after the blinder draw for provers in step, as the parent commit offers it."""
        P = len(provers)
        B = tab.msm_many([job for (_, _, _, C, D, z, c, d, rc, rd) in provers for job in ((G, rc), (Gp, rd))])
        rounds_in, gammas = [], []
        for p, ((_, _, _, C, D, z, c, d, rc, rd), t) in enumerate(zip(provers, ts)):
            t.append_list(b"ipa_step1", comp([C, D]))
            t.append(b"ipa_step1", fr32(z))
            t.append_list(b"ipa_step1", comp(B[2 * p: 2 * p + 2]))
            alpha = t.get_and_append_challenge(b"ipa_alpha")
            beta = t.get_and_append_challenge(b"ipa_beta")
            rounds_in.append((G, Gp, H, [r + alpha * x for r, x in zip(rc, c)], [r + alpha * x for r, x in zip(rd, d)], None, beta))

            def next_gamma(L_C, L_D, R_C, R_D, t=t):
                t.append_list(b"ipa_loop", comp([L_C, L_D, R_C, R_D]))
                return t.get_and_append_challenge(b"ipa_gamma")

            gammas.append(next_gamma)
        res = K.ipa_rounds_many(rounds_in, gammas, table=tab)
        return [proof_bytes(B[2 * p], B[2 * p + 1], *res[p]) for p in range(P)]

    def device(provers, ts):
        return [proof_bytes(*r) for r in K.ipa_prove_device_many(tab, provers, ts)]

    out = {"reps": a.reps, "n": n, "shapes": {}}
    for P, name in (SHAPES if not a.target else [(a.target, "target")]):
        provers = []
        for _ in range(P):
            c, d = vec(), vec()
            C, D = tab.msm(c, G), tab.msm(d, Gp)
            z = Scalar(sum(x._v * y._v for x, y in zip(c, d)) % R)
            provers.append((G, Gp, H, C, D, z, c, d, vec(), vec()))
        comp([x for pr in provers for x in pr[3:5]])                    # C, D normalised once, outside the timed region, for both sides
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
        # the other inversion, and what lane 0 reports
        ctx.set_param("ipa_inv", 1)
        fermat = []
        for rep in range(a.reps + 2):
            ts = mk()
            t0 = time.perf_counter()
            device(provers, ts)
            if rep >= 2:
                fermat.append((time.perf_counter() - t0) * 1e3)
        rec["device_fermat_ms"] = statistics.median(fermat)
        ticks = {}
        for mode, key in ((0, "binary"), (1, "a^(r-2)")):
            ctx.set_param("ipa_inv", mode)
            gi, gpi = list(range(n)) * P, list(range(n, 2 * n)) * P
            flat = lambda k: b"".join(fr32(s) for pr in provers for s in pr[k])
            cd = b"".join(b"".join(comp(pr[3:5])) for pr in provers)
            z32 = b"".join(fr32(pr[5]) for pr in provers)
            states = b"".join(bytes(t.strobe._st.raw) for t in mk())
            with tab._ctx_lock():
                _, _, ck = ctx.ipa_prove_device(tab._tab, n, P, gi, gpi, [2 * n] * P, None, cd, z32, flat(6), flat(7), flat(8), flat(9), states, want_clocks=True)
            steps = ck[3]
            ticks[key] = {"transcript_per_step": round(statistics.mean(ck[4 * p] for p in range(P)) / steps, 1),
                          "inversion_per_round": round(statistics.mean(ck[4 * p + 1] for p in range(P)) / (steps - 1), 1),
                          "whole_step": round(statistics.mean(ck[4 * p + 2] for p in range(P)) / (steps - 1), 1)}
        ctx.set_param("ipa_inv", 0)
        rec["lane0_ticks"] = ticks
        out["shapes"][name] = rec
    tab.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
