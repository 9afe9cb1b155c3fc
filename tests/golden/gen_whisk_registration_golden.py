#!/usr/bin/env python3
"""Record Whisk REGISTRATIONS as the reference makes them: generate_tracker(k) and get_k_commitment(k)
(/root/reference/curdleproofs/curdleproofs/test_curdleproofs.py:759-790) and GenerateWhiskTrackerProof(tracker, k)
(whisk_interface.py:177-190 -> opening.py:33-56), imported unmodified in the build container with a stand-in for the missing Rust wheel
(tests/golden/_backend.py: the pure-Python CPU oracle by default).  The three functions are called, never restated.

Data only -> tests/golden/whisk_registration_vectors.json:
  "cases":    per case k and the two draws r (generate_tracker's) and b (the proof's blinder), 32 bytes little-endian each, with the
              tracker (r_G, k_r_G), the k_commitment and the proof (A | B | s).  Random cases: the draws are read off copies of the
              generator's state.  Prescribed draws (r in {1, r_order - 1}, k = 1 / r): the randint that the reference's random_scalar
              calls answers them for the length of the call, the reference's code untouched.  k in {0, 1, r_order - 1}.
  "sequence": 32 registrations under one random.seed, per validator generate_tracker then GenerateWhiskTrackerProof as the reference's own
              test does, and the next randint(1, r_order - 1) after the loop: it pins that two values were drawn per item.
  "seeded":   a seed, a few indices and the (r, b) that registration_draws_from_seed must derive -- computed here with hashlib alone:
              block(index, d) = SHAKE256(b"whisk_registration_draw" || seed || le64(index) || le32(d)).digest(64), little-endian, mod r_order.

    python tests/golden/gen_whisk_registration_golden.py [--backend oracle|product]
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_shuffle_golden as G  # noqa: E402  (injects the backend, imports the reference)

import curdleproofs.util as ref_util  # noqa: E402
from curdleproofs.test_curdleproofs import generate_tracker, get_k_commitment  # noqa: E402
from curdleproofs.whisk_interface import GenerateWhiskTrackerProof  # noqa: E402

R = G.FR_MODULUS


def scalar(v):
    return G.Scalar.from_le_bytes(v.to_bytes(32, "little"))


def le32(v):
    return v.to_bytes(32, "little").hex()


def register(k):
    """the reference's three calls for one validator, in its test's order"""
    kc = bytes(get_k_commitment(scalar(k)))
    tracker = generate_tracker(scalar(k))
    proof = bytes(GenerateWhiskTrackerProof(tracker, scalar(k)))
    assert len(proof) == 128 and len(kc) == 48
    return {"r_G": bytes(tracker.r_G).hex(), "k_r_G": bytes(tracker.k_r_G).hex(), "k_commitment": kc.hex(), "proof": proof.hex()}


def record_random(name, k):
    st = random.getstate()
    r, b = random.randint(1, R - 1), random.randint(1, R - 1)
    random.setstate(st)
    case = {"name": name, "k": le32(k), "r": le32(r), "b": le32(b)}
    case.update(register(k))
    assert random.randint(1, R - 1) != r                      # both draws were consumed
    return case


def record_prescribed(name, k, r, b):
    """the randint the reference's random_scalar calls (util.py:1, :21-24) hands out r, then b, and nothing else, while the reference runs"""
    queue = [r, b]
    real = ref_util.randint

    def scripted(lo, hi):
        assert (lo, hi) == (1, R - 1)
        return queue.pop(0)

    ref_util.randint = scripted
    try:
        case = {"name": name, "k": le32(k), "r": le32(r), "b": le32(b)}
        case.update(register(k))
    finally:
        ref_util.randint = real
    assert not queue
    return case


def draws_from_seed(seed, index):
    out = []
    for d in (0, 1):
        block = hashlib.shake_256(b"whisk_registration_draw" + seed + index.to_bytes(8, "little") + d.to_bytes(4, "little")).digest(64)
        out.append(int.from_bytes(block, "little") % R)
    return out


def main():
    random.seed(20261021)
    cases = [record_random(f"random {j}", random.randint(1, R - 1)) for j in range(4)]
    for k, nm in ((0, "k = 0"), (1, "k = 1"), (R - 1, "k = r_order - 1")):
        cases.append(record_random(nm, k))
    k, b = random.randint(1, R - 1), random.randint(1, R - 1)
    cases.append(record_prescribed("r = 1", k, 1, b))
    cases.append(record_prescribed("r = r_order - 1", k, R - 1, b))
    cases.append(record_prescribed("r = r_order - 1, b = r_order - 1, k = r_order - 1", R - 1, R - 1, R - 1))
    r = random.randint(1, R - 1)
    cases.append(record_prescribed("k = 1 / r (k_r_G = G)", pow(r, -1, R), r, random.randint(1, R - 1)))
    cases.append(record_prescribed("k = 0, r = 1, b = 1", 0, 1, 1))

    seq_seed = 4242
    random.seed(seq_seed)
    ks = [random.randint(0, R - 1) for _ in range(32)]
    ks[5] = 0
    random.seed(seq_seed + 1)
    items = [register(k) for k in ks]
    next_draw = random.randint(1, R - 1)
    sequence = {"seed": seq_seed + 1, "ks": [le32(k) for k in ks], "items": items, "next_draw": le32(next_draw)}

    seed = hashlib.sha256(b"whisk registration golden seed").digest()
    seeded = {"seed": seed.hex(), "draws": []}
    for index in (0, 1, 2, 255, 256, 65537, (1 << 32) - 1):
        r, b = draws_from_seed(seed, index)
        seeded["draws"].append({"index": index, "r": le32(r), "b": le32(b)})

    path = G._backend.out_path("whisk_registration_vectors.json")
    with open(path, "w") as f:
        json.dump({"generator": "tests/golden/gen_whisk_registration_golden.py (reference test_curdleproofs / whisk_interface; G1Point/Scalar = %s)" % G.BACKEND_MODULE,
                   "backend": G.BACKEND_MODULE, "cases": cases, "sequence": sequence, "seeded": seeded}, f, separators=(",", ":"))
    print([c["name"] for c in cases])
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
