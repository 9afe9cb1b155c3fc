#!/usr/bin/env python3
"""SamePermutationProof.new (same_perm.py:27-72) stand-alone, for the device prover of the same-permutation argument
(prover_kernels.same_permutation_prove_device).

Runs the reference's SamePermutationProof.new, unmodified, over the CPU-oracle backend (tests/golden/_backend.py) on seeded inputs and
records everything the device path takes and everything it must give back:

  per case: ell, n_blinders, crs_G_vec, crs_H_vec, crs_U, vec_a, the permutation, vec_a_blinders, vec_m_blinders, A and M (built as their
  commitments MSM(G, vec_a o permutation) + MSM(H, vec_a_blinders) and MSM(G, permutation) + MSM(H, vec_m_blinders)); every draw in the
  reference's order (generate_blinders is wrapped in curdleproofs.ipa and in curdleproofs.grand_prod: vec_c_blinders, then r, then the
  n - 2 drawn entries of z); what GrandProductProof.new received (B, gprod_result, vec_b_blinders, and vec_b as its SHA-256 over the
  32-byte encodings, in full for n <= 32); the transcript's label and the prefix message appended before the call (so the start state is
  not a fresh one); same_perm_alpha, same_perm_beta and every later challenge; SamePermutationProof.to_bytes(); and one
  get_and_append_challenge(b"after") drawn afterwards, which pins the final transcript state.
One case has the identity permutation, one the reversed one, and (124, 4) has vec_a_blinders ending in two zeros, as the shuffle
argument builds it (curdleproofs.py:73-74).
To keep the file small the bases of the cases with n > 32 are not stored: they are G1 * k with the n + 1 scalars k the case's seed
gives first (`base_scalars` below, asserted here), and the tests derive them.
Data only -> tests/golden/same_permutation_device_vectors.json.

    python tests/golden/gen_same_permutation_device_golden.py [--backend oracle|product]
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
import curdleproofs.same_perm as sp_mod  # noqa: E402
from curdleproofs.util import CURVE_ORDER, G1, generate_blinders, get_permutation, get_random_point, random_scalar  # noqa: E402
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


_new = gp_mod.GrandProductProof.new.__func__


def _gprod_new(cls, **kw):
    SEEN.update({"B": pt(kw["B"]), "gprod_result": fr(kw["gprod_result"]), "vec_b": [fr(s) for s in kw["vec_b"]],
                 "vec_b_blinders": [fr(s) for s in kw["vec_b_blinders"]]})
    return _new(cls, **kw)


ipa_mod.generate_blinders = _drawing
gp_mod.generate_blinders = _drawing
gp_mod.GrandProductProof.new = classmethod(_gprod_new)
assert sp_mod.GrandProductProof is gp_mod.GrandProductProof

# (ell, n_blinders, seed, permutation: "seeded" | "identity" | "reversed")
CASES = [(1, 3, 301, "seeded"), (2, 2, 302, "reversed"), (6, 2, 303, "seeded"), (4, 4, 304, "seeded"), (28, 4, 305, "identity"), (124, 4, 306, "seeded"),
         (508, 4, 307, "seeded")]


def base_scalars(seed, count):
    """The scalars k of the first `count` get_random_point() = G1 * k calls after random.seed(seed) (util.py:21-24, :67-68)."""
    rng = random.Random(seed)
    return [rng.randint(1, CURVE_ORDER - 1) for _ in range(count)]


def one_case(ell, n_blinders, seed, kind):
    random.seed(seed)
    n = ell + n_blinders
    crs_G_vec = [get_random_point() for _ in range(ell)]
    crs_H_vec = [get_random_point() for _ in range(n_blinders)]
    crs_U = get_random_point()
    vec_a = [random_scalar() for _ in range(ell)]
    permutation = list(range(ell))
    if kind == "seeded":
        random.shuffle(permutation)
    elif kind == "reversed":
        permutation.reverse()
    vec_a_blinders = [random_scalar() for _ in range(n_blinders)]
    if (ell, n_blinders) == (124, 4):
        vec_a_blinders[2:] = [Scalar(0), Scalar(0)]                     # curdleproofs.py:73-74
    vec_m_blinders = [random_scalar() for _ in range(n_blinders)]
    A = compute_MSM(crs_G_vec, get_permutation(vec_a, permutation)) + compute_MSM(crs_H_vec, vec_a_blinders)
    M = compute_MSM(crs_G_vec, [Scalar(m) for m in permutation]) + compute_MSM(crs_H_vec, vec_m_blinders)
    label, prefix = b"same_perm_device_%d" % seed, bytes(random.getrandbits(8) for _ in range(40 + seed % 7))
    transcript = G.CurdleproofsTranscript(label)
    transcript.append(b"prefix", prefix)
    rec = {"ell": ell, "n_blinders": n_blinders, "seed": seed, "permutation_kind": kind}
    if n <= 32:
        rec.update({"crs_G_vec": [pt(p) for p in crs_G_vec], "crs_H_vec": [pt(p) for p in crs_H_vec], "crs_U": pt(crs_U)})
    else:
        ks = base_scalars(seed, n + 1)
        assert pt(crs_G_vec[0]) == pt(G1 * Scalar.from_le_bytes(ks[0].to_bytes(32, "little"))) and pt(crs_U) == pt(G1 * Scalar.from_le_bytes(ks[n].to_bytes(32, "little")))
    rec.update({"A": pt(A), "M": pt(M), "vec_a": [fr(s) for s in vec_a], "permutation": permutation, "vec_a_blinders": [fr(s) for s in vec_a_blinders],
                "vec_m_blinders": [fr(s) for s in vec_m_blinders], "label": label.decode(), "prefix_label": "prefix", "prefix": prefix.hex()})
    del DRAWS[:]
    SEEN.clear()
    mark = len(G.CHALLENGES)
    proof = sp_mod.SamePermutationProof.new(list(crs_G_vec), list(crs_H_vec), crs_U, A, M, list(vec_a), list(permutation), list(vec_a_blinders),
                                            list(vec_m_blinders), transcript)
    drawn = G.CHALLENGES[mark:]
    assert [len(d) for d in DRAWS] == [n_blinders, n, n - 2]
    assert [lab for lab, _ in drawn[:4]] == ["same_perm_alpha", "same_perm_beta", "gprod_alpha", "gprod_beta"]
    one = lambda name: [v for lab, v in drawn if lab == name][0]
    raw = bytes(proof.to_bytes())
    assert raw[:48].hex() == SEEN["B"] == pt(proof.B)
    rec.update({"vec_c_blinders": DRAWS[0], "ipa_r": DRAWS[1], "ipa_z_head": DRAWS[2],
                "B": SEEN["B"], "gprod_result": SEEN["gprod_result"], "vec_b_blinders": SEEN["vec_b_blinders"],
                "vec_b_sha256": hashlib.sha256(bytes.fromhex("".join(SEEN["vec_b"]))).hexdigest(),
                "same_perm_alpha": one("same_perm_alpha"), "same_perm_beta": one("same_perm_beta"), "gprod_alpha": one("gprod_alpha"), "gprod_beta": one("gprod_beta"),
                "ipa_alpha": one("ipa_alpha"), "ipa_beta": one("ipa_beta"), "ipa_gammas": [v for lab, v in drawn if lab == "ipa_gamma"],
                "proof": raw.hex(), "after": fr(transcript.get_and_append_challenge(b"after"))})
    lg = n.bit_length() - 1
    if n <= 32:
        rec["vec_b"] = SEEN["vec_b"]
    assert len(raw) == 48 + 48 + 32 + (2 + 4 * lg) * 48 + 64 and len(rec["ipa_gammas"]) == lg
    return rec


def main():
    out = {"generator": "tests/golden/gen_same_permutation_device_golden.py (reference SamePermutationProof.new; G1Point/Scalar = %s)" % G.BACKEND_MODULE,
           "backend": G.BACKEND_MODULE, "cases": [one_case(*c) for c in CASES]}
    path = G._backend.out_path("same_permutation_device_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print([(c["ell"], c["n_blinders"], len(c["proof"]) // 2) for c in out["cases"]])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
