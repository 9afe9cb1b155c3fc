#!/usr/bin/env python3
"""The grand-product argument proved on the device (prover_kernels.grand_product_prove_device_many, csrc/kernels_gprod.h) against the best
path without it, at (ell, n_blinders) = (124, 4) for 1, 8 and 64 provers in step: the whole of GrandProductProof.new
(grand_prod.py:29-119) after its draws, inputs as Python objects in, proof bytes out.

  device     grand_product_prove_device_many: one launch chain, one wait
  yardstick  the host-driven head -- Python ints for the prefix products, the powers of beta, vec_d and the completion of
             generate_ipa_blinders; table.msm_many for the C's, then for the D's; the host transcript -- followed by
             ipa_prove_device_many with the base change as G_prime_coeffs (one launch chain): three waits

Both run in ONE process and ALTERNATE call by call; the figure is the median wall time of the Python call over --reps (>= 30)
repetitions after two warm-ups.  Fresh transcripts are made outside the timed region.  Both sides must produce the same bytes and the
same transcript states (checked once per shape).  One run prints one JSON line; it also carries, per shape, the C entry alone and what
lane 0 of the step kernels (k_gprod_step and k_ipa_step together) reports in shader-clock ticks.

`--summarize a.json b.json c.json` prints the table over three runs: a shape counts as FASTER when the device median (the median of
the runs) lies below the yardstick's by more than the spread (max - min) of the yardstick's own medians.

`--target P` is a short target for `rocprofv3 --kernel-trace --stats`: five device calls for P provers and nothing else;
`--trace-summary kernel_trace.csv` then prints, for the LAST chain of the trace, every kernel's time and the gap before it.

    python tools/gpu_gprod_device_timing.py [--reps 30] > run1.json
    python tools/gpu_gprod_device_timing.py --summarize run1.json run2.json run3.json
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/gpu_gprod_device_timing.py --target 8
    python tools/gpu_gprod_device_timing.py --trace-summary out/*/*_kernel_trace.csv
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, "gprod_new_124_4_1_prover"), (8, "gprod_new_124_4_8_provers"), (64, "gprod_new_124_4_64_provers")]


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
        r = runs[0]["shapes"][s]
        print("%-28s C entry alone %.4f ms; lane 0, ticks per prover: %s" % (s, r["c_entry_ms"], json.dumps(r["lane0_ticks"])))


def trace_summary(path):
    import csv

    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    short = lambda n: n.split("(")[0].split("::")[-1].split("<")[0]
    begins = [i for i, r in enumerate(rows) if "k_gprod_step" in r["Kernel_Name"] and (i == 0 or "k_fixed_finish" not in rows[i - 1]["Kernel_Name"])]
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

    rng = random.Random(21)
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

    def proof_bytes(C, r_p, ipa):
        B_c, B_d, LC, RC, LD, RD, c_fin, d_fin = ipa
        return comp(C) + fr32(r_p) + b"".join(comp(p) for p in [B_c, B_d] + list(LC) + list(RC) + list(LD) + list(RD)) + fr32(c_fin) + fr32(d_fin)

    def host_driven(provers, ts):
        """GrandProductProof.new after its draws for provers in step: the head on the host, then the IPA's device chain."""
        heads = []
        for (_, _, _, B, gres, b, bbl, cbl, r, zh), t in zip(provers, ts):
            t.append(b"gprod_step1", comp(B))
            t.append(b"gprod_step1", fr32(gres))
            alpha = int(t.get_and_append_challenge(b"gprod_alpha"))
            bi, cbi = [int(x) for x in b], [int(x) for x in cbl]
            c = [1]
            for i in range(ell - 1):
                c.append(c[i] * bi[i] % R)
            heads.append((alpha, bi, c + cbi))
        Cs = tab.msm_many([(vec_G, sc(h[2])) for h in heads])
        tails = []
        for (_, _, _, B, gres, b, bbl, cbl, r, zh), t, (alpha, bi, c), C in zip(provers, ts, heads, Cs):
            rba = [(int(x) + alpha) % R for x in bbl]
            r_p = sum(x * y for x, y in zip(rba, c[ell:])) % R
            t.append(b"gprod_step2", comp(C))
            t.append(b"gprod_step2", fr32(Scalar(r_p)))
            beta = int(t.get_and_append_challenge(b"gprod_beta"))
            kgp = K.grand_product_coeffs(ell, nb, Scalar(pow(beta, -1, R)))
            d, pw = [], 1
            for j in range(ell):
                d.append(pw * (bi[j] * beta - 1) % R)
                pw = pw * beta % R
            d += [pw * beta % R * x % R for x in rba]
            inner = (r_p * pw * beta + int(gres) * pw - 1) % R
            ri, zi = [int(x) for x in r], [int(x) for x in zh]
            dot = lambda u, v: sum(x * y for x, y in zip(u, v)) % R
            omega, delta = (dot(ri, d) + dot(zi, c[: n - 2])) % R, dot(ri[: n - 2], zi)
            inv_c = pow(c[n - 2], -1, R)
            last_z = (ri[n - 2] * inv_c * omega - delta) * pow((-ri[n - 2] * inv_c * c[n - 1] + ri[n - 1]) % R, -1, R) % R
            pen_z = -inv_c * (last_z * c[n - 1] + omega) % R
            tails.append((r_p, kgp, d, inner, zi + [pen_z, last_z]))
        Ds = tab.msm_many([(vec_G, sc(x * int(k) % R for x, k in zip(tl[2], tl[1]))) for tl in tails])
        ipa = K.ipa_prove_device_many(tab, [(vec_G, vec_G, U, C, D, Scalar(tl[3]), sc(h[2]), sc(tl[2]), pr[8], sc(tl[4]), tl[1])
                                            for pr, h, tl, C, D in zip(provers, heads, tails, Cs, Ds)], ts)
        return [proof_bytes(C, Scalar(tl[0]), res) for C, tl, res in zip(Cs, tails, ipa)]

    def device(provers, ts):
        return [proof_bytes(*res) for res in K.grand_product_prove_device_many(tab, provers, ts)]

    out = {"reps": a.reps, "ell": ell, "n_blinders": nb, "shapes": {}}
    for P, name in (SHAPES if not a.target else [(a.target, "target")]):
        provers = []
        for _ in range(P):
            b, bbl = vec(ell), vec(nb)
            prod = 1
            for x in b:
                prod = prod * int(x) % R
            provers.append((vec_G[:ell], vec_G[ell:], U, tab.msm(b + bbl, vec_G), Scalar(prod), b, bbl, vec(nb), vec(n), vec(n - 2)))
        M.points_to_affine96([pr[3] for pr in provers])               # normalised once, outside the timed region, for both sides
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
        flat = lambda *ks: b"".join(fr32(s) for pr in provers for k in ks for s in pr[k])
        args = (list(range(n)) * P, [U] * P, b"".join(comp(pr[3]) for pr in provers), b"".join(fr32(pr[4]) for pr in provers), flat(5, 6), flat(7), flat(8), flat(9))
        entry = []
        with tab._ctx_lock():
            for rep in range(a.reps + 2):
                states = b"".join(bytes(t.strobe._st.raw) for t in mk())
                t0 = time.perf_counter()
                _, _, ck = ctx.gprod_prove_device(tab._tab, ell, nb, P, *args, states, want_clocks=True)
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
