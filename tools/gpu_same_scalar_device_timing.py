#!/usr/bin/env python3
"""The shuffle prover's same-scalar block proved on the device (prover_kernels.same_scalar_prove_device_many, csrc/kernels_same_scalar.h)
against the best host-driven paths without it, at ell = 124 for 1, 8 and 64 provers in step: curdleproofs.py:92-116 after the draws -- R, S,
cm_T, cm_U and all of SameScalarProof.new --, inputs as Python objects in, the 576 proof bytes per prover out.

  device_certified   same_scalar_prove_device_many over bases that carry their G1 certificate: 6 launches, one wait
  device_tested      the same over bases decoded unchecked: k_subgroup_row runs inside the chain, 7 launches, one wait
  yardstick          as the reference writes it, batched: compute_MSM_batch for every prover's R and S (one call), then ONE
                     compute_MSM_batch of the eight commitment halves per prover (G_t r_t; R k + H r_t; ...: R and S themselves are
                     multiplied), the host transcript, the responses in Python ints: two round trips
  yardstick_folded   the device chain's algebra driven from the host: k a_i and r_k a_i in Python ints, ONE compute_MSM_batch of ten
                     MSMs per prover over the original bases, the host transcript: one round trip
The verdict is taken against the FASTER of the two yardsticks.

All sides run in ONE process and ALTERNATE call by call; the figure is the median wall time of the Python call over --reps (>= 30)
repetitions after two warm-ups.  Fresh transcripts are made outside the timed region.  All sides must produce the same bytes and the
same transcript states (checked once per shape, before anything is timed).  One run prints one JSON line; it also carries, per shape,
the C entry alone for both settings of bases_certified.

`--summarize a.json b.json c.json` prints the table over three runs: a shape counts as FASTER when the device median (the median of
the runs) lies below the yardstick's by more than the spread (max - min) of the yardstick's own medians.

`--target P` is a short target for `rocprofv3 --kernel-trace --stats`: five device_tested calls for P provers and nothing else;
`--trace-summary kernel_trace.csv` then prints, for the LAST chain of the trace, every kernel's time and the gap before it.

    python tools/gpu_same_scalar_device_timing.py [--reps 30] > run1.json
    python tools/gpu_same_scalar_device_timing.py --summarize run1.json run2.json run3.json
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/gpu_same_scalar_device_timing.py --target 8
    python tools/gpu_same_scalar_device_timing.py --trace-summary out/*/*_kernel_trace.csv
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, "same_scalar_124_1_prover"), (8, "same_scalar_124_8_provers"), (64, "same_scalar_124_64_provers")]
SIDES = ("device_certified", "device_tested", "yardstick", "yardstick_folded")


def summarize(paths):
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    print("%-28s %-17s %10s %-17s %12s %10s %8s  %s" % ("shape", "device side", "device ms", "yardstick", "yardstick ms", "spread ms", "ratio", "verdict"))
    for _, s in SHAPES:
        med = {side: [r["shapes"][s][side + "_ms"] for r in runs] for side in SIDES}
        best = min(("yardstick", "yardstick_folded"), key=lambda side: statistics.median(med[side]))
        ys = med[best]
        y, spread = statistics.median(ys), max(ys) - min(ys)
        for side in ("device_certified", "device_tested"):
            f = statistics.median(med[side])
            verdict = "FASTER" if f < y - spread else ("slower" if f > y + spread else "no difference")
            print("%-28s %-17s %10.4f %-17s %12.4f %10.4f %7.2fx  %s   (device runs: %s; yardstick runs: %s)" %
                  (s, side, f, best, y, spread, y / f, verdict, " ".join("%.4f" % v for v in med[side]), " ".join("%.4f" % v for v in ys)))
        other = "yardstick_folded" if best == "yardstick" else "yardstick"
        print("%-28s the other yardstick, %s: %s ms" % (s, other, " ".join("%.4f" % v for v in med[other])))
    for _, s in SHAPES:
        r = runs[0]["shapes"][s]
        print("%-28s C entry alone: certified %.4f ms, tested %.4f ms; light table %d bases" % (s, r["c_entry_certified_ms"], r["c_entry_tested_ms"], r["light_bases"]))


def trace_summary(path):
    import csv

    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    short = lambda n: n.split("(")[0].split("<")[0].split("::")[-1]
    steps = [i for i, r in enumerate(rows) if "k_sscalar_step" in r["Kernel_Name"]]
    chain = rows[steps[-2]: steps[-1] + 1]                               # begin .. step of the last call
    t0 = int(chain[0]["Start_Timestamp"])
    print("the last chain of %s: %d launches, %.1f us from the first kernel's start to the last one's end" %
          (os.path.basename(path), len(chain), (int(chain[-1]["End_Timestamp"]) - t0) / 1e3))
    print("%4s %-18s %10s %10s %10s" % ("#", "kernel", "start us", "time us", "gap us"))
    prev_end = None
    for i, r in enumerate(chain):
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        gap = 0.0 if prev_end is None else (s - prev_end) / 1e3
        print("%4d %-18s %10.1f %10.1f %10.1f" % (i, short(r["Kernel_Name"]), (s - t0) / 1e3, (e - s) / 1e3, gap))
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
    from curdleproofs_pie_amd import _native as N

    N.tune_runtime()
    from curdleproofs_pie_amd import msm_accumulator as M
    from curdleproofs_pie_amd import prover_kernels as K
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.py_arkworks_bls12381 import CURVE_ORDER as R, G1Point, Scalar, points_to_affine96

    rng = random.Random(23)
    ell = 124
    rs = lambda: Scalar(rng.randint(1, R - 1))
    vec = lambda m: [rs() for _ in range(m)]
    comp = lambda p: bytes(p.to_compressed_bytes())
    fr32 = lambda s: bytes(s.to_le_bytes())
    crs = [G1Point.from_compressed_bytes(comp(p)) for p in M.batch_mul([G1Point()] * 3, vec(3))]
    Gt, Gu, H = crs
    tab = FixedBaseTable(crs)
    ctx = N.default_context()

    def finish(points, provers, ts):
        """The host transcript and the responses over each prover's ten points in the transcript's order -> the 576 bytes."""
        out = []
        for p, (pr, t) in enumerate(zip(provers, ts)):
            enc = [comp(x) for x in points[10 * p: 10 * p + 10]]
            t.append_list(b"sameexp_points", enc)
            alpha = int(t.get_and_append_challenge(b"same_scalar_alpha"))
            k, r_t, r_u, r_a, r_b, r_k = (int(x) for x in pr[6:12])
            z = [(r_k + k * alpha) % R, (r_a + r_t * alpha) % R, (r_b + r_u * alpha) % R]
            out.append(b"".join(enc[2:6] + enc[0:2] + enc[6:10]) + b"".join(v.to_bytes(32, "little") for v in z))
        return out

    def yardstick(provers, ts):
        RS = M.compute_MSM_batch([(list(v), list(pr[5])) for pr in provers for v in (pr[3], pr[4])])
        jobs, order = [], []
        for p, pr in enumerate(provers):
            Rp, Sp = RS[2 * p], RS[2 * p + 1]
            k, r_t, r_u, r_a, r_b, r_k = pr[6:12]
            for G, T, f, r in ((Gt, Rp, k, r_t), (Gu, Sp, k, r_u), (Gt, Rp, r_k, r_a), (Gu, Sp, r_k, r_b)):
                jobs.append(([G], [r])); jobs.append(([T, H], [f, r]))
        C = M.compute_MSM_batch(jobs)
        for p in range(len(provers)):
            order += [RS[2 * p], RS[2 * p + 1]] + C[8 * p: 8 * p + 8]
        return finish(order, provers, ts)

    def yardstick_folded(provers, ts):
        jobs = []
        for pr in provers:
            vR, vS, va = list(pr[3]), list(pr[4]), list(pr[5])
            k, r_t, r_u, r_a, r_b, r_k = pr[6:12]
            ai = [int(x) for x in va]
            ka, rka = [Scalar(int(k) * x % R) for x in ai], [Scalar(int(r_k) * x % R) for x in ai]
            jobs += [(vR, va), (vS, va), ([Gt], [r_t]), (vR + [H], ka + [r_t]), ([Gu], [r_u]), (vS + [H], ka + [r_u]),
                     ([Gt], [r_a]), (vR + [H], rka + [r_a]), ([Gu], [r_b]), (vS + [H], rka + [r_b])]
        return finish(M.compute_MSM_batch(jobs), provers, ts)

    def proof_bytes(res):
        R_, S_, cm_T, cm_U, cm_A, cm_B, z_k, z_t, z_u = res
        return b"".join(comp(p) for p in [*cm_T, *cm_U, R_, S_, *cm_A, *cm_B]) + fr32(z_k) + fr32(z_t) + fr32(z_u)

    def device(provers, ts):
        return [proof_bytes(res) for res in K.same_scalar_prove_device_many(tab, provers, ts)]

    out = {"reps": a.reps, "ell": ell, "shapes": {}}
    for P, name in (SHAPES if not a.target else [(a.target, "target")]):
        pts = [comp(p) for p in M.batch_mul([G1Point()] * (2 * ell * P), vec(2 * ell * P))]
        cert = [G1Point.from_compressed_bytes(e) for e in pts]           # carry their certificate
        unk = [G1Point.from_compressed_bytes_unchecked(e) for e in pts]  # membership not known: the chain tests them
        assert all(x._sg is True for x in cert) and all(x._sg is None for x in unk)
        points_to_affine96(cert + unk)                                   # normalised once, outside the timed region, for all sides
        tails = [(vec(ell), *vec(6)) for _ in range(P)]
        mk_provers = lambda objs: [(Gt, Gu, H, objs[2 * ell * p: 2 * ell * p + ell], objs[2 * ell * p + ell: 2 * ell * (p + 1)], *tails[p]) for p in range(P)]
        provers = {"device_certified": mk_provers(cert), "device_tested": mk_provers(unk), "yardstick": mk_provers(cert), "yardstick_folded": mk_provers(cert)}
        fns = {"device_certified": device, "device_tested": device, "yardstick": yardstick, "yardstick_folded": yardstick_folded}
        mk = lambda: [CurdleproofsTranscript(b"timing %d" % p) for p in range(P)]
        if a.target:
            for _ in range(5):
                device(provers["device_tested"], mk())
            tab.close()
            return
        first = None
        for side in SIDES:                                               # the bytes and the states are compared first
            ts = mk()
            got = (fns[side](provers[side], ts), [bytes(t.strobe._st.raw) for t in ts])
            first = first or got
            assert got == first, (name, side)
        assert all(x._sg is None for x in unk)                           # no host test ran on the device_tested side
        samples = {side: [] for side in SIDES}
        for rep in range(a.reps + 2):                                    # two warm-ups, then the sides alternate
            for side in SIDES:
                ts = mk()
                t0 = time.perf_counter()
                fns[side](provers[side], ts)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= 2:
                    samples[side].append(dt)
        rec = {side + "_ms": statistics.median(samples[side]) for side in SIDES}
        # the C entry alone (arguments already packed), both settings
        gth, rs96 = bytes(points_to_affine96(crs)), bytes(points_to_affine96(cert))
        flat = lambda vals: b"".join(fr32(s) for s in vals)
        args = (gth, rs96, flat(x for t in tails for x in t[0]), flat(t[1] for t in tails), flat(x for t in tails for x in t[2:7]))
        for certified in (True, False):
            entry = []
            with tab._ctx_lock():
                for rep in range(a.reps + 2):
                    states = b"".join(bytes(t.strobe._st.raw) for t in mk())
                    t0 = time.perf_counter()
                    ctx.same_scalar_prove_device(tab._tab, ell, P, *args, certified, states)
                    if rep >= 2:
                        entry.append((time.perf_counter() - t0) * 1e3)
            rec["c_entry_%s_ms" % ("certified" if certified else "tested")] = statistics.median(entry)
        rec["light_bases"] = 3 + P * 2 * ell
        out["shapes"][name] = rec
    tab.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
