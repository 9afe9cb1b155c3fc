#!/usr/bin/env python3
"""IPA.new (ipa.py:75-153) stand-alone, for the device prover of the inner-product argument (prover_kernels.ipa_prove_device).

Runs the reference's IPA.new, unmodified, over the CPU-oracle backend (tests/golden/_backend.py) on seeded inputs and records
everything the device path takes and everything it must give back:

  per case: n, crs_G_vec, crs_G_prime_vec (explicit points, or -- the coefficient form -- the bases G with beta_inv, G'_i = G_i beta^-(i+1),
  the grand-product base change grand_prod.py:64-71), crs_H, C, D, z, vec_c, vec_d, the blinders generate_ipa_blinders drew (captured
  through a wrapper; the draws stay the reference's), the transcript's label and the prefix message appended before IPA.new (so the
  start state is not a fresh one), IPA.to_bytes() of the proof, the ipa_alpha / ipa_beta / ipa_gamma challenges, and one
  get_and_append_challenge(b"after") drawn after IPA.new, which pins the final transcript state.
Data only -> tests/golden/ipa_device_vectors.json.

    python tests/golden/gen_ipa_device_golden.py [--backend oracle|product]
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_shuffle_golden as G  # noqa: E402  (injects the backend, imports the reference, records challenges)

import curdleproofs.ipa as ipa_mod  # noqa: E402
from curdleproofs.util import get_random_point, inner_product, random_scalar  # noqa: E402
from curdleproofs.msm_accumulator import compute_MSM  # noqa: E402

pt = lambda p: bytes(G.point_projective_to_bytes(p)).hex()
fr = lambda s: bytes(s.to_le_bytes()).hex()

BLINDERS = {}
_gen = ipa_mod.generate_ipa_blinders


def _capturing(c, d):
    r_c, r_d = _gen(c, d)
    BLINDERS["r_c"], BLINDERS["r_d"] = [fr(s) for s in r_c], [fr(s) for s in r_d]
    return r_c, r_d


ipa_mod.generate_ipa_blinders = _capturing

CASES = [(2, False, 101), (8, False, 102), (32, False, 103), (128, False, 104), (8, True, 105), (128, True, 106)]


def one_case(n, coeff_form, seed):
    random.seed(seed)
    crs_G_vec = [get_random_point() for _ in range(n)]
    crs_H = get_random_point()
    rec = {"n": n, "seed": seed, "form": "coeffs" if coeff_form else "explicit", "crs_G_vec": [pt(p) for p in crs_G_vec], "crs_H": pt(crs_H)}
    if coeff_form:
        beta_inv = random_scalar()
        crs_G_prime_vec, p = [], beta_inv
        for g in crs_G_vec:                                   # grand_prod.py:64-71
            crs_G_prime_vec.append(g * p)
            p = p * beta_inv
        rec["beta_inv"] = fr(beta_inv)
    else:
        crs_G_prime_vec = [get_random_point() for _ in range(n)]
    rec["crs_G_prime_vec"] = [pt(p) for p in crs_G_prime_vec]
    vec_c = [random_scalar() for _ in range(n)]
    vec_d = [random_scalar() for _ in range(n)]
    z = inner_product(vec_c, vec_d)
    C = compute_MSM(crs_G_vec, vec_c)
    D = compute_MSM(crs_G_prime_vec, vec_d)
    label, prefix = b"ipa_device_%d" % seed, bytes(random.getrandbits(8) for _ in range(40 + seed % 7))
    transcript = G.CurdleproofsTranscript(label)
    transcript.append(b"prefix", prefix)
    rec.update({"C": pt(C), "D": pt(D), "z": fr(z), "vec_c": [fr(s) for s in vec_c], "vec_d": [fr(s) for s in vec_d],
                "label": label.decode(), "prefix_label": "prefix", "prefix": prefix.hex()})
    mark = len(G.CHALLENGES)
    proof = ipa_mod.IPA.new(list(crs_G_vec), list(crs_G_prime_vec), crs_H, C, D, z, list(vec_c), list(vec_d), transcript)
    drawn = G.CHALLENGES[mark:]
    rec.update({"vec_r_c": BLINDERS["r_c"], "vec_r_d": BLINDERS["r_d"], "proof": bytes(proof.to_bytes()).hex(),
                "alpha": [v for lab, v in drawn if lab == "ipa_alpha"][0], "beta": [v for lab, v in drawn if lab == "ipa_beta"][0],
                "gammas": [v for lab, v in drawn if lab == "ipa_gamma"],
                "after": fr(transcript.get_and_append_challenge(b"after"))})
    lg = n.bit_length() - 1
    assert len(rec["proof"]) // 2 == (2 + 4 * lg) * 48 + 64 and len(rec["gammas"]) == lg
    return rec


def main():
    out = {"generator": "tests/golden/gen_ipa_device_golden.py (reference IPA.new; G1Point/Scalar = %s)" % G.BACKEND_MODULE, "backend": G.BACKEND_MODULE,
           "cases": [one_case(*c) for c in CASES]}
    path = G._backend.out_path("ipa_device_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print([(c["n"], c["form"], len(c["proof"]) // 2) for c in out["cases"]])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
