#!/usr/bin/env python3
"""Whole GenerateWhiskShuffleProof calls of the reference, for the batched prover from tracker bytes (shuffle_prover.ShuffleBatchProver).

Runs the reference's GenerateWhiskShuffleProof (whisk_interface.py:111-140), unmodified, over the CPU-oracle backend
(tests/golden/_backend.py).  Per case (ell = 4 and 12): a CRS and two lists of pre-shuffle trackers made under `setup_seed`; then
random.seed(seed) and the two calls, one after the other.  Recorded: both seeds, the CRS point encodings, the pre-trackers, what each call
returned (post-trackers and whisk_shuffle_proof_bytes), and one random.random() drawn after the second call -- the state a batched
prover that draws like the reference must leave `random` in.  The reference's verifier accepts every proof (asserted here).
Data only -> tests/golden/whisk_shuffle_prover_vectors.json.

    python tests/golden/gen_whisk_shuffle_prover_golden.py [--backend oracle|product]
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_shuffle_golden as G  # noqa: E402  (injects the backend, imports the reference)

pt = lambda p: bytes(G.point_projective_to_bytes(p)).hex()
trk = lambda ts: [[bytes(t.r_G).hex(), bytes(t.k_r_G).hex()] for t in ts]

# (ell, setup_seed, seed)
CASES = [(4, 1501, 2501), (12, 1502, 2502)]


def one_case(ell, setup_seed, seed):
    random.seed(setup_seed)
    crs = G.CurdleproofsCrs.new(ell, G.N_BLINDERS)
    lists = [G.make_trackers(ell), G.make_trackers(ell)]
    random.seed(seed)
    outs = [G.GenerateWhiskShuffleProof(crs, pre) for pre in lists]
    after = random.random()
    for pre, (post, proof) in zip(lists, outs):
        assert G.IsValidWhiskShuffleProof(crs, pre, post, proof)
    return {"ell": ell, "setup_seed": setup_seed, "seed": seed,
            "vec_G": [pt(p) for p in crs.vec_G], "vec_H": [pt(p) for p in crs.vec_H], "H": pt(crs.H), "G_t": pt(crs.G_t), "G_u": pt(crs.G_u),
            "G_sum": pt(crs.G_sum), "H_sum": pt(crs.H_sum),
            "pre_trackers": [trk(pre) for pre in lists], "post_trackers": [trk(post) for post, _ in outs], "proofs": [bytes(proof).hex() for _, proof in outs],
            "random_after": repr(after)}


def main():
    out = {"generator": "tests/golden/gen_whisk_shuffle_prover_golden.py (reference GenerateWhiskShuffleProof; G1Point/Scalar = %s)" % G.BACKEND_MODULE,
           "backend": G.BACKEND_MODULE, "cases": [one_case(*c) for c in CASES]}
    path = G._backend.out_path("whisk_shuffle_prover_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print([(c["ell"], [len(p) // 2 for p in c["proofs"]]) for c in out["cases"]])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
