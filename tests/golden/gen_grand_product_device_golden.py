#!/usr/bin/env python3
"""GrandProductProof.new (grand_prod.py:29-119) stand-alone, for the device prover of the grand-product argument
(prover_kernels.grand_product_prove_device).

Runs the reference's GrandProductProof.new, unmodified, over the CPU-oracle backend (tests/golden/_backend.py) on seeded inputs and records
everything the device path takes and everything it must give back:

  per case: ell, n_blinders, crs_G_vec, crs_H_vec, crs_U, B (built as the commitment MSM(G, b) + MSM(H, b_blinders)), gprod_result,
  vec_b, vec_b_blinders; every draw in the reference's order (generate_blinders is wrapped in curdleproofs.ipa and in
  curdleproofs.grand_prod: vec_c_blinders, then r, then the n - 2 drawn entries of z) and the two entries generate_ipa_blinders added
  to z (it returned r unchanged and z with its head unchanged: asserted here); what IPA.new received (C, D, z, and vec_d as its
  SHA-256 over the 32-byte encodings, in full for n <= 32); the transcript's label and the prefix message appended before the call
  (so the start state is not a fresh one); gprod_alpha, gprod_beta and the IPA's challenges; GrandProductProof.to_bytes(); and one
  get_and_append_challenge(b"after") drawn afterwards, which pins the final transcript state.
To keep the file small the bases of the cases with n > 32 are not stored: they are G1 * k with the n + 1 scalars k the case's seed
gives first (`base_scalars` below, asserted here), and the tests derive them.
Data only -> tests/golden/grand_product_device_vectors.json.

    python tests/golden/gen_grand_product_device_golden.py [--backend oracle|product]
"""
import hashlib
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_shuffle_golden as G  # noqa: E402  (injects the backend, imports the reference, records challenges)

import curdleproofs.grand_prod as gp_mod  # noqa: E402
import curdleproofs.ipa as ipa_mod  # noqa: E402
from curdleproofs.util import CURVE_ORDER, G1, generate_blinders, get_random_point, random_scalar  # noqa: E402
from curdleproofs.msm_accumulator import compute_MSM  # noqa: E402
from py_arkworks_bls12381 import Scalar  # noqa: E402

pt = lambda p: bytes(G.point_projective_to_bytes(p)).hex()
fr = lambda s: bytes(s.to_le_bytes()).hex()

DRAWS = []                                                     # every generate_blinders call of a case, in order
SEEN = {}


def _drawing(n):
    out = generate_blinders(n)
    DRAWS.append([fr(s) for s in out])
    return out


_gen = ipa_mod.generate_ipa_blinders


def _capturing(c, d):
    r_c, r_d = _gen(c, d)
    SEEN["r_c"], SEEN["r_d"] = [fr(s) for s in r_c], [fr(s) for s in r_d]
    return r_c, r_d


_new = ipa_mod.IPA.new.__func__


def _ipa_new(cls, **kw):
    SEEN.update({"C": pt(kw["C"]), "D": pt(kw["D"]), "z": fr(kw["z"]), "vec_d": [fr(s) for s in kw["vec_d"]]})
    return _new(cls, **kw)


ipa_mod.generate_blinders = _drawing
gp_mod.generate_blinders = _drawing
ipa_mod.generate_ipa_blinders = _capturing
ipa_mod.IPA.new = classmethod(_ipa_new)

CASES = [(1, 3, 201), (2, 2, 202), (6, 2, 203), (4, 4, 204), (28, 4, 205), (124, 4, 206), (508, 4, 207)]


def base_scalars(seed, count):
    """The scalars k of the first `count` get_random_point() = G1 * k calls after random.seed(seed) (util.py:21-24, :67-68)."""
    rng = random.Random(seed)
    return [rng.randint(1, CURVE_ORDER - 1) for _ in range(count)]


def one_case(ell, n_blinders, seed):
    random.seed(seed)
    n = ell + n_blinders
    crs_G_vec = [get_random_point() for _ in range(ell)]
    crs_H_vec = [get_random_point() for _ in range(n_blinders)]
    crs_U = get_random_point()
    vec_b = [random_scalar() for _ in range(ell)]
    vec_b_blinders = [random_scalar() for _ in range(n_blinders)]
    B = compute_MSM(crs_G_vec, vec_b) + compute_MSM(crs_H_vec, vec_b_blinders)
    gprod_result = Scalar(1)
    for b in vec_b:
        gprod_result = gprod_result * b
    label, prefix = b"gprod_device_%d" % seed, bytes(random.getrandbits(8) for _ in range(40 + seed % 7))
    transcript = G.CurdleproofsTranscript(label)
    transcript.append(b"prefix", prefix)
    rec = {"ell": ell, "n_blinders": n_blinders, "seed": seed}
    if n <= 32:
        rec.update({"crs_G_vec": [pt(p) for p in crs_G_vec], "crs_H_vec": [pt(p) for p in crs_H_vec], "crs_U": pt(crs_U)})
    else:
        ks = base_scalars(seed, n + 1)
        assert pt(crs_G_vec[0]) == pt(G1 * Scalar.from_le_bytes(ks[0].to_bytes(32, "little"))) and pt(crs_U) == pt(G1 * Scalar.from_le_bytes(ks[n].to_bytes(32, "little")))
    rec.update({"B": pt(B), "gprod_result": fr(gprod_result), "vec_b": [fr(s) for s in vec_b],
                "vec_b_blinders": [fr(s) for s in vec_b_blinders], "label": label.decode(), "prefix_label": "prefix", "prefix": prefix.hex()})
    del DRAWS[:]
    SEEN.clear()
    mark = len(G.CHALLENGES)
    proof = gp_mod.GrandProductProof.new(list(crs_G_vec), list(crs_H_vec), crs_U, B, gprod_result, list(vec_b), list(vec_b_blinders), transcript)
    drawn = G.CHALLENGES[mark:]
    assert [len(d) for d in DRAWS] == [n_blinders, n, n - 2]
    one = lambda name: [v for lab, v in drawn if lab == name][0]
    assert SEEN["r_c"] == DRAWS[1] and SEEN["r_d"][: n - 2] == DRAWS[2]
    rec.update({"vec_c_blinders": DRAWS[0], "ipa_r": DRAWS[1], "ipa_z_head": DRAWS[2], "ipa_z_tail": SEEN["r_d"][n - 2:],
                "ipa_C": SEEN["C"], "ipa_D": SEEN["D"], "ipa_z": SEEN["z"], "vec_d_sha256": hashlib.sha256(bytes.fromhex("".join(SEEN["vec_d"]))).hexdigest(),
                "gprod_alpha": one("gprod_alpha"), "gprod_beta": one("gprod_beta"), "ipa_alpha": one("ipa_alpha"), "ipa_beta": one("ipa_beta"),
                "ipa_gammas": [v for lab, v in drawn if lab == "ipa_gamma"], "proof": bytes(proof.to_bytes()).hex(),
                "after": fr(transcript.get_and_append_challenge(b"after"))})
    lg = n.bit_length() - 1
    if n <= 32:
        rec["vec_d"] = SEEN["vec_d"]
    assert len(rec["proof"]) // 2 == 48 + 32 + (2 + 4 * lg) * 48 + 64 and len(rec["ipa_gammas"]) == lg
    return rec


def main():
    out = {"generator": "tests/golden/gen_grand_product_device_golden.py (reference GrandProductProof.new; G1Point/Scalar = %s)" % G.BACKEND_MODULE,
           "backend": G.BACKEND_MODULE, "cases": [one_case(*c) for c in CASES]}
    path = G._backend.out_path("grand_product_device_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print([(c["ell"], c["n_blinders"], len(c["proof"]) // 2) for c in out["cases"]])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
