#!/usr/bin/env python3
"""What tests/golden/prover_vectors.json leaves out of IPA.new's inputs: crs_H itself and the challenge beta (the fixture records only
their product H = crs_H * beta, ipa.py:110), for the fixed-base tables -- a table holds CRS points, so a prover hands `crs_H` plus the
coefficient beta to prover_kernels.ipa_rounds(..., H_coeff=beta, table=tab).

Runs the very flow of gen_prover_golden.py (the reference's GenerateWhiskShuffleProof, unmodified, over the CPU-oracle backend, same
seed), checks that the IPA record it reproduces is the committed one, and writes the two missing values.
Data only -> tests/golden/fixed_base_vectors.json.

    python tests/golden/gen_fixed_base_golden.py [--backend oracle|product]
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_prover_golden as GP  # noqa: E402  (injects the backend, imports the reference, wraps IPA.new / SameMSMProof.new)

G = GP.G
EXTRA = {}
_wrapped = GP.ipa_mod.IPA.new.__func__


def ipa_new(cls, crs_G_vec, crs_G_prime_vec, crs_H, C, D, z, vec_c, vec_d, transcript):
    mark = len(G.CHALLENGES)
    proof = _wrapped(cls, crs_G_vec, crs_G_prime_vec, crs_H, C, D, z, vec_c, vec_d, transcript)
    EXTRA["ipa_crs_H"] = GP.pt(crs_H)
    EXTRA["ipa_beta"] = GP.challenges_since(mark, "ipa_beta")[0]
    return proof


GP.ipa_mod.IPA.new = classmethod(ipa_new)


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ell = 28
    random.seed(4711)
    crs = G.CurdleproofsCrs.new(ell, G.N_BLINDERS)
    pre = G.make_trackers(ell)
    del G.CHALLENGES[:]
    post, proof = G.GenerateWhiskShuffleProof(crs, pre)
    assert G.IsValidWhiskShuffleProof(crs, pre, post, proof)
    with open(os.path.join(here, "prover_vectors.json")) as f:
        committed = json.load(f)
    assert GP.REC["ipa"] == committed["ipa"], "this run is not the run prover_vectors.json records"
    out ={"generator": "tests/golden/gen_fixed_base_golden.py (reference prover; G1Point/Scalar = %s)" % G.BACKEND_MODULE, "backend": G.BACKEND_MODULE,
           "ell": ell, "H": committed["ipa"]["H"], **EXTRA}
    path = G._backend.out_path("fixed_base_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
