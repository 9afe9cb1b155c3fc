#!/usr/bin/env python3
"""Record the fixture of tests/test_shuffle_verifier.py::test_differential_against_reference_verifier: one seeded proof
(ell = 12) from the reference prover, EVERY field of the proof and both ends of every tracker buffer tampered in turn, and
the verdict the reference verifier (IsValidWhiskShuffleProof, whisk_interface.py:72-109) returned for each.  Same shape as
a case of shuffle_vectors.json (gen_shuffle_golden.py, whose imports and helpers this uses); written to
tests/golden/differential_vectors.json -- data only.

    python tests/golden/gen_differential_golden.py [--backend oracle|product] [--out PATH]
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _backend  # noqa: E402
import gen_shuffle_golden as G  # noqa: E402   (injects the backend, imports the reference)


def main():
    rng = random.Random(2024)
    random.seed(77)
    ell = 12
    crs = G.CurdleproofsCrs.new(ell, 4)
    pre = G.make_trackers(ell)
    post, proof = G.GenerateWhiskShuffleProof(crs, pre)
    proof = bytes(proof)
    offs, total = G.proof_offsets(4)
    assert total == len(proof)
    other = bytes(G.point_projective_to_bytes(G.G1 * G.Scalar(12345)))
    pre_r, pre_k = G.cat(pre)
    post_r, post_k = G.cat(post)
    base = {"proof": proof, "pre_r": pre_r, "pre_k": pre_k, "post_r": post_r, "post_k": post_k}
    variants = []

    def push(name, edits):
        b = G.apply_edits(base, edits)
        accepts = bool(G.IsValidWhiskShuffleProof(crs, G.split(b["pre_r"], b["pre_k"]), G.split(b["post_r"], b["post_k"]), b["proof"]))
        variants.append({"name": name, "edits": edits, "accepts": accepts})

    push("valid", [])
    push("trailing bytes", [["proof", len(proof), "00" * 7]])
    for nm, (off, size) in offs.items():
        if size == 48:
            push(nm + " := other", [["proof", off, other.hex()]])
        else:
            val = (int.from_bytes(proof[off: off + 32], "little") + rng.randint(1, 1000)) % G.FR_MODULUS
            push(nm + " shifted", [["proof", off, val.to_bytes(32, "little").hex()]])
    for which, key in enumerate(("pre_r", "pre_k", "post_r", "post_k")):
        for idx in (0, ell - 1):
            push(f"tracker buf {which}[{idx}] := other", [[key, 48 * idx, other.hex()]])
    out = {"generator": "tests/golden/gen_differential_golden.py (reference whisk_interface; G1Point/Scalar = %s)" % G.BACKEND_MODULE,
           "backend": G.BACKEND_MODULE, "ell": ell, "crs": bytes(crs.to_bytes()).hex(), **{k: v.hex() for k, v in base.items()},
           "variants": variants}
    path = _backend.out_path("differential_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("variants", [(v["name"], v["accepts"]) for v in variants])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
