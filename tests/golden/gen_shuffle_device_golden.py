#!/usr/bin/env python3
"""Whole shuffle proofs of the reference prover, for the device prover of the whole proof (prover_kernels.shuffle_prove_device).

Runs the reference's shuffle_permute_and_commit_input and CurdleProofsProof.new, unmodified, over the CPU-oracle backend
(tests/golden/_backend.py) on seeded inputs and records everything the device path takes and everything it must give back:

  per case: ell, the CRS points, vec_R, vec_S, the permutation, k; what shuffle_permute_and_commit_input returned (vec_T, vec_U, M,
  vec_m_blinders); every random draw of CurdleProofsProof.new in the order the reference makes it (random_scalar is wrapped in
  curdleproofs.util -- which generate_blinders calls -- and in the two modules that import it by name, curdleproofs.curdleproofs and
  curdleproofs.same_scalar: the draws stay the reference's) cut into vec_a_blinders (2) | vec_c_blinders (4) | ipa_r (n) | ipa_z_head
  (n - 2) | r_t, r_u | r_a, r_b, r_k | vec_r (n); the first and the last challenge curdleproofs_vec_a (a check of the transcript head); and
  the full CurdleProofsProof.to_bytes().  The reference's verify accepts every proof (asserted here).
To keep the file small the bases of the cases with ell > 32 are not stored: they are G1 * k with the ell + 7 + 2 ell scalars k the case's
seed gives first (`base_scalars` below, asserted here), in the order vec_G, vec_H, H, G_t, G_u, vec_R, vec_S, and the tests derive them.
Data only -> tests/golden/shuffle_device_vectors.json.

    python tests/golden/gen_shuffle_device_golden.py [--backend oracle|product]
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_shuffle_golden as G  # noqa: E402  (injects the backend, imports the reference, records challenges)

import curdleproofs.curdleproofs as cp_mod  # noqa: E402
import curdleproofs.same_scalar as ss_mod  # noqa: E402
import curdleproofs.util as util_mod  # noqa: E402
from curdleproofs.crs import CurdleproofsCrs  # noqa: E402
from curdleproofs.util import CURVE_ORDER, G1, get_random_point, random_scalar  # noqa: E402
from py_arkworks_bls12381 import Scalar  # noqa: E402

pt = lambda p: bytes(G.point_projective_to_bytes(p)).hex()
fr = lambda s: bytes(s.to_le_bytes()).hex()

N_BLINDERS = cp_mod.N_BLINDERS
DRAWS = []                                                     # every random_scalar call while RECORDING, in order
RECORDING = [False]
_draw = util_mod.random_scalar


def _drawing():
    s = _draw()
    if RECORDING[0]:
        DRAWS.append(fr(s))
    return s


util_mod.random_scalar = _drawing                              # generate_blinders (util.py:81-82) looks it up at every call
cp_mod.random_scalar = _drawing
ss_mod.random_scalar = _drawing

# (ell, seed, permutation: "seeded" | "identity" | "reversed")
CASES = [(4, 501, "identity"), (12, 502, "reversed"), (28, 503, "seeded"), (124, 504, "seeded")]


def base_scalars(seed, count):
    """The scalars k of the first `count` get_random_point() = G1 * k calls after random.seed(seed) (util.py:21-24, :67-68)."""
    rng = random.Random(seed)
    return [rng.randint(1, CURVE_ORDER - 1) for _ in range(count)]


def one_case(ell, seed, kind):
    random.seed(seed)
    n = ell + N_BLINDERS
    crs = CurdleproofsCrs.new(ell, N_BLINDERS)
    vec_R = [get_random_point() for _ in range(ell)]
    vec_S = [get_random_point() for _ in range(ell)]
    k = random_scalar()
    permutation = list(range(ell))
    if kind == "seeded":
        random.shuffle(permutation)
    elif kind == "reversed":
        permutation.reverse()
    vec_T, vec_U, M, vec_m_blinders = cp_mod.shuffle_permute_and_commit_input(crs, vec_R, vec_S, permutation, k)
    rec = {"ell": ell, "seed": seed, "permutation_kind": kind, "permutation": permutation, "k": fr(k)}
    if ell <= 32:
        rec.update({"vec_G": [pt(p) for p in crs.vec_G], "vec_H": [pt(p) for p in crs.vec_H], "H": pt(crs.H), "G_t": pt(crs.G_t), "G_u": pt(crs.G_u),
                    "vec_R": [pt(p) for p in vec_R], "vec_S": [pt(p) for p in vec_S]})
    else:
        ks = base_scalars(seed, n + 3 + 2 * ell)
        mul = lambda v: pt(G1 * Scalar.from_le_bytes(v.to_bytes(32, "little")))
        assert pt(crs.vec_G[0]) == mul(ks[0]) and pt(crs.vec_H[0]) == mul(ks[ell]) and pt(crs.H) == mul(ks[n]) and pt(crs.G_u) == mul(ks[n + 2])
        assert pt(vec_R[0]) == mul(ks[n + 3]) and pt(vec_S[-1]) == mul(ks[n + 2 + 2 * ell])
    rec.update({"vec_T": [pt(p) for p in vec_T], "vec_U": [pt(p) for p in vec_U], "M": pt(M), "vec_m_blinders": [fr(s) for s in vec_m_blinders]})
    del DRAWS[:]
    mark = len(G.CHALLENGES)
    RECORDING[0] = True
    proof = cp_mod.CurdleProofsProof.new(crs, list(vec_R), list(vec_S), list(vec_T), list(vec_U), M, list(permutation), k, list(vec_m_blinders))
    RECORDING[0] = False
    vec_a = [v for lab, v in G.CHALLENGES[mark:] if lab == "curdleproofs_vec_a"]
    assert len(vec_a) == ell and len(DRAWS) == 2 + N_BLINDERS + n + (n - 2) + 2 + 3 + n
    cut, at = {}, 0
    for name, count in (("vec_a_blinders", 2), ("vec_c_blinders", N_BLINDERS), ("ipa_r", n), ("ipa_z_head", n - 2), ("r_t", 0), ("r_u", 0), ("r_a", 0), ("r_b", 0),
                        ("r_k", 0), ("vec_r", n)):
        cut[name] = DRAWS[at: at + count] if count else DRAWS[at]
        at += count or 1
    proof.verify(crs, vec_R, vec_S, vec_T, vec_U, M)            # raises when the reference's verifier rejects
    raw = bytes(proof.to_bytes())
    lg = n.bit_length() - 1
    assert len(raw) == 48 + 288 + (48 + 48 + 32 + (2 + 4 * lg) * 48 + 64) + 288 + (3 + 6 * lg) * 48 + 32
    rec.update({"draws": cut, "vec_a_first": vec_a[0], "vec_a_last": vec_a[-1], "proof": raw.hex()})
    return rec


def main():
    out = {"generator": "tests/golden/gen_shuffle_device_golden.py (reference shuffle_permute_and_commit_input, CurdleProofsProof.new; G1Point/Scalar = %s)" % G.BACKEND_MODULE,
           "backend": G.BACKEND_MODULE, "cases": [one_case(*c) for c in CASES]}
    path = G._backend.out_path("shuffle_device_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print([(c["ell"], len(c["proof"]) // 2) for c in out["cases"]])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
