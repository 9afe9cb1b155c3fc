#!/usr/bin/env python3
"""The same-MSM argument proved on the device (prover_kernels.same_msm_prove_device_many, csrc/kernels_same_msm.h) against the
host-driven path it would replace, at n = 128 for 1, 8 and 64 provers in step: the whole of SameMSMProof.new (same_msm.py:75-143) after
the blinder draw, inputs as Python objects in, proof bytes out.

  device     same_msm_prove_device_many: one launch chain (the light table over T | U built inside it), one wait
  yardstick  the host-driven path: compute_MSM_batch for B_a / B_t / B_u, the host transcript, same_msm_rounds_many, the points compressed

Both run in ONE process and ALTERNATE call by call; the figure is the median wall time of the Python call over --reps (>= 30)
repetitions after two warm-ups.  Fresh transcripts are made outside the timed region.  Both sides must produce the same bytes and the
same transcript states (checked once per shape).  One run prints one JSON line; it also carries, per shape, what lane 0 of k_smsm_step
reports about its serial part (shader-clock ticks in the transcript and in the inversion of gamma, per step).

`--summarize a.json b.json c.json` prints the table over three runs: a shape counts as FASTER when the device median (the median of
the runs) lies below the yardstick's by more than the spread (max - min) of the yardstick's own medians.

`--target P` is a short target for `rocprofv3 --kernel-trace --stats`: five device calls for P provers and nothing else;
`--trace-summary kernel_trace.csv` then prints, for the LAST chain of the trace, every kernel's time and the gap before it.

    python tools/gpu_same_msm_device_timing.py [--reps 30] > run1.json
    python tools/gpu_same_msm_device_timing.py --summarize run1.json run2.json run3.json
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/gpu_same_msm_device_timing.py --target 8
    python tools/gpu_same_msm_device_timing.py --trace-summary out/*/*_kernel_trace.csv
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, "same_msm_new_n128_1_prover"), (8, "same_msm_new_n128_8_provers"), (64, "same_msm_new_n128_64_provers")]


def summarize(paths):
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    print("%-30s %12s %12s %10s %10s  %s" % ("shape", "device ms", "yardstick ms", "spread ms", "ratio", "verdict"))
    for _, s in SHAPES:
        dv = [r["shapes"][s]["device_ms"] for r in runs]
        ys = [r["shapes"][s]["yardstick_ms"] for r in runs]
        f, y, spread = statistics.median(dv), statistics.median(ys), max(ys) - min(ys)
        verdict = "FASTER" if f < y - spread else ("slower" if f > y + spread else "no difference")
        print("%-30s %12.4f %12.4f %10.4f %9.2fx  %s   (device runs: %s; yardstick runs: %s)" %
              (s, f, y, spread, y / f, verdict, " ".join("%.4f" % v for v in dv), " ".join("%.4f" % v for v in ys)))
    for _, s in SHAPES:
        for r in runs[:1]:
            print("%-30s lane 0 per step, ticks: %s" % (s, json.dumps(r["shapes"][s]["lane0_ticks"])))


def trace_summary(path):
    import csv

    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    short = lambda n: n.split("(")[0].split("::")[-1]
    begins = [i for i, r in enumerate(rows) if "k_smsm_step" in r["Kernel_Name"] and (i == 0 or "k_fixed_finish" not in rows[i - 1]["Kernel_Name"])]
    chain = rows[begins[-1]:]
    last = max(i for i, r in enumerate(chain) if "k_smsm_step" in r["Kernel_Name"])
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

    rng = random.Random(18)
    n = 128
    rs = lambda: Scalar(rng.randint(1, R - 1))
    vec = lambda: [rs() for _ in range(n)]
    G = M.batch_mul([G1Point()] * n, vec())
    M.points_to_affine96(G)
    tab = FixedBaseTable(G)
    ctx = N.default_context()
    comp = lambda ps: [bytes(p.to_compressed_bytes()) for p in ps]
    fr32 = lambda s: bytes(s.to_le_bytes())

    def proof_bytes(B_a, B_t, B_u, LA, LT, LU, RA, RT, RU, x_fin):
        return b"".join(comp([B_a, B_t, B_u] + list(LA) + list(LT) + list(LU) + list(RA) + list(RT) + list(RU))) + fr32(x_fin)

    def host_driven(provers, ts):
        """SameMSMProof.new after the blinder draw for provers in step, as the parent commit offers it."""
        P = len(provers)
        B = M.compute_MSM_batch([job for (_, A, Zt, Zu, T, U, x, r) in provers for job in ((G, r), (T, r), (U, r))])
        rounds_in, gammas = [], []
        for p, ((_, A, Zt, Zu, T, U, x, r), t) in enumerate(zip(provers, ts)):
            t.append_list(b"same_msm_step1", comp([A, Zt, Zu]))
            t.append_list(b"same_msm_step1", comp(T + U))
            t.append_list(b"same_msm_step1", comp(B[3 * p: 3 * p + 3]))
            alpha = t.get_and_append_challenge(b"same_msm_alpha")
            rounds_in.append((G, T, U, [ri + alpha * xi for ri, xi in zip(r, x)]))

            def next_gamma(*pts, t=t):
                t.append_list(b"same_msm_loop", comp(pts))
                return t.get_and_append_challenge(b"same_msm_gamma")

            gammas.append(next_gamma)
        res = K.same_msm_rounds_many(rounds_in, gammas)
        return [proof_bytes(*B[3 * p: 3 * p + 3], *res[p]) for p in range(P)]

    def device(provers, ts):
        return [proof_bytes(*r) for r in K.same_msm_prove_device_many(tab, provers, ts)]

    out = {"reps": a.reps, "n": n, "shapes": {}}
    for P, name in (SHAPES if not a.target else [(a.target, "target")]):
        provers = []
        for _ in range(P):
            TU = M.batch_mul([G1Point()] * (2 * n), [rs() for _ in range(2 * n)])
            T, U, x = TU[:n], TU[n:], vec()
            A, Zt, Zu = M.compute_MSM_batch([(G, x), (T, x), (U, x)])
            provers.append((G, A, Zt, Zu, T, U, x, vec()))
        M.points_to_affine96([q for pr in provers for q in list(pr[1:4]) + pr[4] + pr[5]])      # normalised once, outside the timed region, for both sides
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
        azz = b"".join(b"".join(comp(pr[1:4])) for pr in provers)
        tu = b"".join(bytes(M.points_to_affine96(pr[4] + pr[5])) for pr in provers)
        x32, r32, gi = flat(6), flat(7), list(range(n)) * P
        entry = []
        with tab._ctx_lock():
            for rep in range(a.reps + 2):
                states = b"".join(bytes(t.strobe._st.raw) for t in mk())
                t0 = time.perf_counter()
                _, _, ck = ctx.same_msm_prove_device(tab._tab, n, P, gi, azz, tu, x32, r32, states, want_clocks=True)
                if rep >= 2:
                    entry.append((time.perf_counter() - t0) * 1e3)
        rec["c_entry_ms"] = statistics.median(entry)
        steps = ck[3]
        rec["lane0_ticks"] = {"transcript_per_step": round(statistics.mean(ck[4 * p] for p in range(P)) / steps, 1),
                              "inversion_per_round": round(statistics.mean(ck[4 * p + 1] for p in range(P)) / (steps - 1), 1),
                              "whole_step": round(statistics.mean(ck[4 * p + 2] for p in range(P)) / (steps - 1), 1)}
        out["shapes"][name] = rec
    tab.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
