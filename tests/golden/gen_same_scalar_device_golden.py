#!/usr/bin/env python3
"""The shuffle prover's same-scalar block (curdleproofs.py:92-116) stand-alone, for its device prover
(prover_kernels.same_scalar_prove_device).

Runs the reference's own calls of that block, unmodified, over the CPU-oracle backend (tests/golden/_backend.py) on seeded inputs --
R = compute_MSM(vec_R, vec_a), S = compute_MSM(vec_S, vec_a), cm_T = GroupCommitment.new(G_t, H, R * k, r_t),
cm_U = GroupCommitment.new(G_u, H, S * k, r_u), SameScalarProof.new(...) -- and records everything the device path takes and everything it
must give back:

  per case: ell, crs_G_t, crs_G_u, crs_H, vec_R, vec_S, vec_a, k, the draws r_t, r_u (made here, where curdleproofs.py:92-93 makes them)
  and r_a, r_b, r_k (random_scalar is wrapped in curdleproofs.same_scalar: the draws stay the reference's, in its order); the transcript's
  label and the prefix message appended before the block (so the start state is not a fresh one); same_scalar_alpha; the 576 bytes
  cm_T | cm_U | R | S | cm_A | cm_B | z_k | z_t | z_u (CurdleProofsProof.to_bytes order, curdleproofs.py:283-297, without A, M and the other
  arguments' proofs); and one get_and_append_challenge(b"after") drawn afterwards, which pins the final transcript state.
To keep the file small the bases of the cases with ell > 32 are not stored: they are G1 * k with the 2 ell + 3 scalars k the case's seed
gives first (`base_scalars` below, asserted here), in the order G_t, G_u, H, vec_R, vec_S, and the tests derive them.
Data only -> tests/golden/same_scalar_device_vectors.json.

    python tests/golden/gen_same_scalar_device_golden.py [--backend oracle|product]
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_shuffle_golden as G  # noqa: E402  (injects the backend, imports the reference, records challenges)

import curdleproofs.same_scalar as ss_mod  # noqa: E402
from curdleproofs.commitment import GroupCommitment  # noqa: E402
from curdleproofs.util import CURVE_ORDER, G1, get_random_point, random_scalar  # noqa: E402
from curdleproofs.msm_accumulator import compute_MSM  # noqa: E402
from py_arkworks_bls12381 import Scalar  # noqa: E402

pt = lambda p: bytes(G.point_projective_to_bytes(p)).hex()
fr = lambda s: bytes(s.to_le_bytes()).hex()

DRAWS = []                                                     # SameScalarProof.new's random_scalar calls of a case, in order
_draw = ss_mod.random_scalar


def _drawing():
    s = _draw()
    DRAWS.append(fr(s))
    return s


ss_mod.random_scalar = _drawing

# (ell, seed)
CASES = [(1, 401), (2, 402), (5, 403), (8, 404), (28, 405), (124, 406)]


def base_scalars(seed, count):
    """The scalars k of the first `count` get_random_point() = G1 * k calls after random.seed(seed) (util.py:21-24, :67-68)."""
    rng = random.Random(seed)
    return [rng.randint(1, CURVE_ORDER - 1) for _ in range(count)]


def one_case(ell, seed):
    random.seed(seed)
    crs_G_t, crs_G_u, crs_H = get_random_point(), get_random_point(), get_random_point()
    vec_R = [get_random_point() for _ in range(ell)]
    vec_S = [get_random_point() for _ in range(ell)]
    vec_a = [random_scalar() for _ in range(ell)]
    k = random_scalar()
    label, prefix = b"same_scalar_device_%d" % seed, bytes(random.getrandbits(8) for _ in range(40 + seed % 7))
    transcript = G.CurdleproofsTranscript(label)
    transcript.append(b"prefix", prefix)
    rec = {"ell": ell, "seed": seed}
    if ell <= 32:
        rec.update({"crs_G_t": pt(crs_G_t), "crs_G_u": pt(crs_G_u), "crs_H": pt(crs_H), "vec_R": [pt(p) for p in vec_R], "vec_S": [pt(p) for p in vec_S]})
    else:
        ks = base_scalars(seed, 2 * ell + 3)
        mul = lambda v: pt(G1 * Scalar.from_le_bytes(v.to_bytes(32, "little")))
        assert pt(crs_G_t) == mul(ks[0]) and pt(crs_H) == mul(ks[2]) and pt(vec_R[0]) == mul(ks[3]) and pt(vec_S[-1]) == mul(ks[2 * ell + 2])
    rec.update({"vec_a": [fr(s) for s in vec_a], "k": fr(k), "label": label.decode(), "prefix_label": "prefix", "prefix": prefix.hex()})
    del DRAWS[:]
    mark = len(G.CHALLENGES)
    # ---- curdleproofs.py:92-116
    r_t = random_scalar()
    r_u = random_scalar()
    R = compute_MSM(vec_R, vec_a)
    S = compute_MSM(vec_S, vec_a)
    cm_T = GroupCommitment.new(crs_G_t, crs_H, R * k, r_t)
    cm_U = GroupCommitment.new(crs_G_u, crs_H, S * k, r_u)
    proof = ss_mod.SameScalarProof.new(crs_G_t=crs_G_t, crs_G_u=crs_G_u, crs_H=crs_H, R=R, S=S, cm_T=cm_T, cm_U=cm_U, k=k, r_t=r_t, r_u=r_u, transcript=transcript)
    drawn = G.CHALLENGES[mark:]
    assert len(DRAWS) == 3 and [lab for lab, _ in drawn] == ["same_scalar_alpha"]
    # curdleproofs.py:283-297 between M and the same-permutation proof, then the same-scalar proof
    raw = b"".join([bytes(cm_T.to_bytes()), bytes(cm_U.to_bytes()), bytes(G.point_projective_to_bytes(R)), bytes(G.point_projective_to_bytes(S)), bytes(proof.to_bytes())])
    assert len(raw) == 576
    rec.update({"r_t": fr(r_t), "r_u": fr(r_u), "r_a": DRAWS[0], "r_b": DRAWS[1], "r_k": DRAWS[2], "alpha": drawn[0][1], "proof": raw.hex(),
                "after": fr(transcript.get_and_append_challenge(b"after"))})
    return rec


def main():
    out = {"generator": "tests/golden/gen_same_scalar_device_golden.py (reference curdleproofs.py:92-116, SameScalarProof.new; G1Point/Scalar = %s)" % G.BACKEND_MODULE,
           "backend": G.BACKEND_MODULE, "cases": [one_case(*c) for c in CASES]}
    path = G._backend.out_path("same_scalar_device_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print([(c["ell"], len(c["proof"]) // 2) for c in out["cases"]])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
