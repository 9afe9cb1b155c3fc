#!/usr/bin/env python3
"""SameMSMProof.new (same_msm.py:50-143) stand-alone, for the device prover of the same-MSM argument
(prover_kernels.same_msm_prove_device).

Runs the reference's SameMSMProof.new, unmodified, over the CPU-oracle backend (tests/golden/_backend.py) on seeded inputs and records
everything the device path takes and everything it must give back:

  per case: n, crs_G_vec, vec_T, vec_U, vec_x, A = MSM(G, x), Z_t = MSM(T, x), Z_u = MSM(U, x), the blinders generate_blinders drew
  (captured through a wrapper; the draws stay the reference's), the transcript's label and the prefix message appended before
  SameMSMProof.new (so the start state is not a fresh one), SameMSMProof.to_bytes() of the proof, the same_msm_alpha / same_msm_gamma
  challenges, and one get_and_append_challenge(b"after") drawn after it, which pins the final transcript state.
  Shapes: "random" -- T and U random points; "shuffle" -- the shuffle argument's own (curdleproofs.py:124-136): T ends in Z1, Z1, H, Z1
  and U in Z1, Z1, Z1, H, with H also one of the CRS bases (crs_G_vec[0]).
Data only -> tests/golden/same_msm_device_vectors.json.

    python tests/golden/gen_same_msm_device_golden.py [--backend oracle|product]
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_shuffle_golden as G  # noqa: E402  (injects the backend, imports the reference, records challenges)

import curdleproofs.same_msm as sm_mod  # noqa: E402
from curdleproofs.util import Z1, get_random_point, random_scalar  # noqa: E402
from curdleproofs.msm_accumulator import compute_MSM  # noqa: E402

pt = lambda p: bytes(G.point_projective_to_bytes(p)).hex()
fr = lambda s: bytes(s.to_le_bytes()).hex()

BLINDERS = {}
_gen = sm_mod.generate_blinders


def _capturing(n):
    r = _gen(n)
    BLINDERS["r"] = [fr(s) for s in r]
    return r


sm_mod.generate_blinders = _capturing

CASES = [(2, "random", 201), (8, "random", 202), (32, "random", 203), (128, "random", 204), (8, "shuffle", 205), (128, "shuffle", 206)]


def one_case(n, shape, seed):
    random.seed(seed)
    crs_G_vec = [get_random_point() for _ in range(n)]
    if shape == "shuffle":
        H = crs_G_vec[0]
        vec_T = [get_random_point() for _ in range(n - 4)] + [Z1, Z1, H, Z1]
        vec_U = [get_random_point() for _ in range(n - 4)] + [Z1, Z1, Z1, H]
    else:
        vec_T = [get_random_point() for _ in range(n)]
        vec_U = [get_random_point() for _ in range(n)]
    vec_x = [random_scalar() for _ in range(n)]
    A, Z_t, Z_u = compute_MSM(crs_G_vec, vec_x), compute_MSM(vec_T, vec_x), compute_MSM(vec_U, vec_x)
    label, prefix = b"same_msm_device_%d" % seed, bytes(random.getrandbits(8) for _ in range(40 + seed % 7))
    transcript = G.CurdleproofsTranscript(label)
    transcript.append(b"prefix", prefix)
    rec = {"n": n, "seed": seed, "shape": shape, "crs_G_vec": [pt(p) for p in crs_G_vec], "vec_T": [pt(p) for p in vec_T], "vec_U": [pt(p) for p in vec_U],
           "vec_x": [fr(s) for s in vec_x], "A": pt(A), "Z_t": pt(Z_t), "Z_u": pt(Z_u), "label": label.decode(), "prefix_label": "prefix",
           "prefix": prefix.hex()}
    mark = len(G.CHALLENGES)
    proof = sm_mod.SameMSMProof.new(list(crs_G_vec), A, Z_t, Z_u, list(vec_T), list(vec_U), list(vec_x), transcript)
    drawn = G.CHALLENGES[mark:]
    rec.update({"vec_r": BLINDERS["r"], "proof": bytes(proof.to_bytes()).hex(), "alpha": [v for lab, v in drawn if lab == "same_msm_alpha"][0],
                "gammas": [v for lab, v in drawn if lab == "same_msm_gamma"], "after": fr(transcript.get_and_append_challenge(b"after"))})
    lg = n.bit_length() - 1
    assert len(rec["proof"]) // 2 == (3 + 6 * lg) * 48 + 32 and len(rec["gammas"]) == lg and len(rec["vec_r"]) == n
    return rec


def main():
    out = {"generator": "tests/golden/gen_same_msm_device_golden.py (reference SameMSMProof.new; G1Point/Scalar = %s)" % G.BACKEND_MODULE,
           "backend": G.BACKEND_MODULE, "cases": [one_case(*c) for c in CASES]}
    path = G._backend.out_path("same_msm_device_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print([(c["n"], c["shape"], len(c["proof"]) // 2) for c in out["cases"]])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
