#!/usr/bin/env python3
"""Record Whisk tracker-opening proofs as the reference PROVER makes them: GenerateWhiskTrackerProof
(/root/reference/curdleproofs/curdleproofs/whisk_interface.py:177-190 -> opening.py:33-56), imported unmodified in the build
container with a stand-in for the missing Rust wheel (tests/golden/_backend.py: the pure-Python CPU oracle by default), on seeded inputs.

Data only -> tests/golden/opening_prover_vectors.json:
  "cases":    per case r_G, k_r_G, k (32 bytes little-endian), the blinder the reference drew, k_commitment = G1 * k and the proof
              (A | B | s) -- or "raises": true where GenerateWhiskTrackerProof raised ValueError (no blinder is drawn then).  Random
              trackers, the identity tracker, r_G on the curve but outside G1 (T3 = (0, 2), order 3), k_r_G != k r_G, k in {0, 1, r - 1},
              bad encodings in r_G and in k_r_G (flags, x >= p, x^3 + 4 not a square);
  "sequence": 32 calls in a row under one random.seed (two bad trackers among them, the reference loop catching ValueError), the
              proofs (null where it raised) and the next randint(1, r - 1) after the loop: it pins how many blinders were drawn.

    python tests/golden/gen_opening_prover_golden.py [--backend oracle|product]
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_shuffle_golden as G  # noqa: E402  (injects the backend, imports the reference)

from curdleproofs.whisk_interface import GenerateWhiskTrackerProof  # noqa: E402
from py_arkworks_bls12381 import G1Point  # noqa: E402

R = G.FR_MODULUS
IDENTITY = b"\xc0" + bytes(47)
T3 = bytes([0x80]) + bytes(47)                                  # x = 0, y = 2: on the curve, order 3
BAD_FLAGS = b"\x00" + bytes(47)                                 # compression flag missing
X_TOO_BIG = bytes([0x9f]) + b"\xff" * 47                        # x >= p


def pb(p):
    return bytes(G.point_projective_to_bytes(p))


def scalar(v):
    return G.Scalar.from_le_bytes(v.to_bytes(32, "little"))


def not_on_curve():
    """the first x = 1, 2, ... with x^3 + 4 not a square mod p, encoded with the compression flag"""
    for x in range(1, 100):
        enc = bytes([0x80]) + x.to_bytes(47, "big")
        try:
            G1Point.from_compressed_bytes_unchecked(enc)
        except Exception:
            return enc
    raise RuntimeError("no non-square found")


def record(name, r_G, k_r_G, k):
    """one GenerateWhiskTrackerProof call; the blinder it draws is read off a copy of the generator's state"""
    st = random.getstate()
    blinder = random.randint(1, R - 1)
    random.setstate(st)
    tracker = G.WhiskTracker(G.BLSPubkey(r_G), G.BLSPubkey(k_r_G))
    case = {"name": name, "r_G": r_G.hex(), "k_r_G": k_r_G.hex(), "k": k.to_bytes(32, "little").hex()}
    try:
        proof = bytes(GenerateWhiskTrackerProof(tracker, scalar(k)))
    except ValueError:
        random.setstate(st)
        assert random.randint(1, R - 1) == blinder
        random.setstate(st)                                     # no draw happened: the state is where it was
        case["raises"] = True
        return case
    assert len(proof) == 128
    case.update(blinder=blinder.to_bytes(32, "little").hex(), k_commitment=pb(G.G1 * scalar(k)).hex(), proof=proof.hex())
    return case


def main():
    random.seed(20261016)
    cases = []
    for j in range(4):
        k, r = random.randint(1, R - 1), random.randint(1, R - 1)
        r_G = G.G1 * scalar(r)
        cases.append(record(f"random {j}", pb(r_G), pb(r_G * scalar(k)), k))
    k = random.randint(1, R - 1)
    cases.append(record("r_G = identity", IDENTITY, IDENTITY, k))
    cases.append(record("r_G = identity, junk after the flags", b"\xe0" + bytes(46) + b"\x05", IDENTITY, k))
    t3 = G1Point.from_compressed_bytes_unchecked(T3)
    cases.append(record("r_G = T3 (outside G1)", T3, pb(t3 * scalar(k)), k))
    r_G = G.G1 * scalar(random.randint(1, R - 1)) + t3
    cases.append(record("r_G = P + T3 (outside G1)", pb(r_G), pb(r_G * scalar(k)), k))
    r_G = G.G1 * scalar(random.randint(1, R - 1))
    cases.append(record("k_r_G != k r_G", pb(r_G), pb(G.G1 * scalar(random.randint(1, R - 1))), k))
    for kk, nm in ((1, "k = 1"), (R - 1, "k = r - 1"), (0, "k = 0")):
        cases.append(record(nm, pb(r_G), pb(r_G * scalar(kk)), kk))
    good = pb(r_G)
    for bad, nm in ((BAD_FLAGS, "bad flags"), (X_TOO_BIG, "x >= p"), (not_on_curve(), "not on the curve")):
        cases.append(record(f"r_G: {nm}", bad, good, k))
        cases.append(record(f"k_r_G: {nm}", good, bad, k))
    # one seeded sequence of calls, two bad trackers mixed in (the caller's loop catches ValueError)
    seq_seed = 777
    random.seed(seq_seed)
    items = []
    for j in range(32):
        kj, rj = random.randint(1, R - 1), random.randint(1, R - 1)
        rG = G.G1 * scalar(rj)
        tr = (pb(rG), pb(rG * scalar(kj)))
        if j == 7:
            tr = (BAD_FLAGS, tr[1])
        if j == 20:
            tr = (tr[0], X_TOO_BIG)
        items.append((tr, kj))
    random.seed(seq_seed + 1)
    proofs = []
    for (r_b, kr_b), kj in items:
        try:
            proofs.append(bytes(GenerateWhiskTrackerProof(G.WhiskTracker(G.BLSPubkey(r_b), G.BLSPubkey(kr_b)), scalar(kj))).hex())
        except ValueError:
            proofs.append(None)
    next_draw = random.randint(1, R - 1)
    sequence = {"seed": seq_seed + 1, "items": [{"r_G": r_b.hex(), "k_r_G": kr_b.hex(), "k": kj.to_bytes(32, "little").hex()} for (r_b, kr_b), kj in items],
                "proofs": proofs, "next_draw": next_draw.to_bytes(32, "little").hex()}
    path = G._backend.out_path("opening_prover_vectors.json")
    with open(path, "w") as f:
        json.dump({"generator": "tests/golden/gen_opening_prover_golden.py (reference whisk_interface; G1Point/Scalar = %s)" % G.BACKEND_MODULE,
                   "backend": G.BACKEND_MODULE, "cases": cases, "sequence": sequence}, f, separators=(",", ":"))
    print([(c["name"], "raises" if c.get("raises") else "ok") for c in cases])
    print("sequence:", sum(p is None for p in proofs), "raised of", len(proofs))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
