#!/usr/bin/env python3
"""Shuffle proofs that carry a point outside the prime-order subgroup in the same-scalar equalities, with the reference verifier's
verdicts, at the smallest size the protocol admits (ell = 4, n = 8) -- and one accepted such proof at ell = 124 over the CRS of
tests/golden/shuffle_batch_ell124.bin, which tools/gpu_exact_device_timing.py puts among that fixture's honest proofs.

Reference classes, unmodified, over the pure-Python oracle backend (tests/golden/_backend.py), driven as gen_torsion_golden.py drives them:
  honest                  two honest proofs
  T3 on <point>           an honest proof whose wire bytes carry <point> + T3, for each of the ten points the verifier watches (T_1 T_2 U_1
                          U_2 R S cm_A.T_1 cm_A.T_2 cm_B.T_1 cm_B.T_2): whatever the reference decides is recorded (it rejects: the
                          point is absorbed by the transcript and stands in an equality that held without the defect)
  cancelling              cm_T.T_1 + T3, cm_U.T_1 - T3, cm_A.T_1 - a T3, cm_B.T_1 + a T3 with a = alpha mod 3: the exact equalities hold and
                          A' = A + T_1 + U_1 has no torsion part -- the reference ACCEPTS
Data only -> tests/golden/exact_device_vectors.json.

    python tests/golden/gen_exact_device_golden.py [--skip-ell124]
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_torsion_golden as T  # noqa: E402  (injects the backend, imports the reference, arms the provers)

G = T.G
from curdleproofs.util import BufReader  # noqa: E402
from py_arkworks_bls12381 import G1Point  # noqa: E402

WATCHED = ("T_1", "T_2", "U_1", "U_2", "R", "S", "cmA_1", "cmA_2", "cmB_1", "cmB_2")


def with_t3(proof: bytes, off: int) -> bytes:
    p = G1Point.from_compressed_bytes_unchecked(proof[off: off + 48]) + T.t3()
    return proof[:off] + T.pb(p) + proof[off + 48:]


def main():
    random.seed(1904)
    ell = 4
    lg = (ell + G.N_BLINDERS).bit_length() - 1
    crs = G.CurdleproofsCrs.new(ell, G.N_BLINDERS)
    offs, total = G.proof_offsets(lg)
    cases = [T.shuffle_case("honest", ell, crs, False), T.shuffle_case("honest 2", ell, crs, False)]
    base = T.shuffle_case("honest 3", ell, crs, False)
    proof = bytes.fromhex(base["proof"])
    assert base["accepts"] and len(proof) == total
    pre, post = G.split(bytes.fromhex(base["pre_r"]), bytes.fromhex(base["pre_k"])), G.split(bytes.fromhex(base["post_r"]), bytes.fromhex(base["post_k"]))
    for name in WATCHED:
        edited = with_t3(proof, offs[name][0])
        accepts = bool(G.IsValidWhiskShuffleProof(crs, pre, post, edited))
        cases.append(dict(base, name=f"T3 on {name}", proof=edited.hex(), accepts=accepts))
    for i in range(4):
        cases.append(T.cancelling_shuffle_case(f"cancelling T3 on cm_T / cm_U / cm_A / cm_B ({i + 1})", ell, crs, want_nonzero=i % 2 == 1))
    out = {"generator": "tests/golden/gen_exact_device_golden.py (reference classes; G1Point/Scalar = %s)" % G.BACKEND_MODULE, "backend": G.BACKEND_MODULE,
           "t3": T.T3_BYTES.hex(), "watched": list(WATCHED), "shuffle": {"ell": ell, "crs": bytes(crs.to_bytes()).hex(), "cases": cases}}
    if "--skip-ell124" not in sys.argv:
        here = os.path.dirname(os.path.abspath(__file__))
        meta = json.load(open(os.path.join(here, "shuffle_batch_ell124.json")))
        crs124 = G.CurdleproofsCrs.from_bytes(BufReader(open(os.path.join(here, "shuffle_batch_ell124.bin"), "rb").read()[: meta["crs_bytes"]]), meta["ell"], meta["n_blinders"])
        random.seed(1905)
        out["ell124"] = T.cancelling_shuffle_case("cancelling T3 at ell = 124 over the CRS of shuffle_batch_ell124", meta["ell"], crs124, want_nonzero=True)
        assert out["ell124"]["accepts"]
    path = G._backend.out_path("exact_device_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("shuffle:", [(c["name"], c["accepts"]) for c in cases])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
