"""Whisk tracker-opening proofs GENERATED in batches (curdleproofs_pie_amd.opening_prover) on the host twin (cg1_opening_prove): every
byte against the reference prover's own output (tests/golden/opening_prover_vectors.json, gen_opening_prover_golden.py), the seeded
call sequence with its blinder draws, the status codes of bad items, seed-derived blinders and generator multiples against the CPU oracle."""
import hashlib
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import bls12_381 as O  # noqa: E402
from oracle import c_oracle  # noqa: E402

R = O.R


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "opening_prover_vectors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def P(native_lib):
    from curdleproofs_pie_amd import opening_prover

    return opening_prover


def case_item(c):
    return (bytes.fromhex(c["r_G"]), bytes.fromhex(c["k_r_G"])), int.from_bytes(bytes.fromhex(c["k"]), "little")


def g96(k):
    pt = O.g1_mul(O.G1_GEN, k % R)
    return bytes(96) if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def test_fixture_bytes_with_recorded_blinders(P, gold):
    prover = P.OpeningBatchProver(device=False)
    for c in gold["cases"]:
        (r, kr), k = case_item(c)
        bl = int.from_bytes(bytes.fromhex(c["blinder"]), "little") if "blinder" in c else 1
        out = prover.prove_many([((r, kr), k)], blinders=[bl])[0]
        if c.get("raises"):
            assert out is None, c["name"]
            assert prover.last_status == [P.BAD_POINT], c["name"]
        else:
            assert out == bytes.fromhex(c["proof"]), c["name"]
            assert prover.last_k_commitments[0] == bytes.fromhex(c["k_commitment"]), c["name"]


def test_fixture_bytes_packed(P, gold):
    ok = [c for c in gold["cases"] if not c.get("raises")]
    trk = b"".join(bytes.fromhex(c["r_G"]) + bytes.fromhex(c["k_r_G"]) for c in ok)
    ks = b"".join(bytes.fromhex(c["k"]) for c in ok)
    bl = b"".join(bytes.fromhex(c["blinder"]) for c in ok)
    proofs, kcs, status = P.OpeningBatchProver(device=False).prove_packed(trk, ks, bl)
    assert status == [0] * len(ok)
    assert proofs == b"".join(bytes.fromhex(c["proof"]) for c in ok)
    assert kcs == b"".join(bytes.fromhex(c["k_commitment"]) for c in ok)


def test_fixture_bytes_with_drawn_blinders(P, gold):
    """no blinders given: the one draw per item goes through randint(1, r - 1) of the caller's generator, as random_scalar does"""
    for c in gold["cases"]:
        if c.get("raises"):
            continue
        want_b = int.from_bytes(bytes.fromhex(c["blinder"]), "little")

        class One:
            def randint(self, a, b):
                assert (a, b) == (1, R - 1)
                return want_b

        assert P.OpeningBatchProver(device=False).prove_many([case_item(c)], rng=One())[0] == bytes.fromhex(c["proof"]), c["name"]


def test_seeded_sequence_same_proofs_and_next_draw(P, gold):
    seq = gold["sequence"]
    items = [((bytes.fromhex(it["r_G"]), bytes.fromhex(it["k_r_G"])), int.from_bytes(bytes.fromhex(it["k"]), "little")) for it in seq["items"]]
    saved = random.getstate()
    try:
        random.seed(seq["seed"])
        prover = P.OpeningBatchProver(device=False)
        got = prover.prove_many(items)
        nxt = random.randint(1, R - 1)
    finally:
        random.setstate(saved)
    assert [g.hex() if g is not None else None for g in got] == seq["proofs"]
    assert nxt.to_bytes(32, "little").hex() == seq["next_draw"]
    assert [s != 0 for s in prover.last_status] == [p is None for p in seq["proofs"]]


def test_bad_items_draw_nothing_and_get_codes(P, gold):
    bad = [c for c in gold["cases"] if c.get("raises")]
    good = next(c for c in gold["cases"] if not c.get("raises"))
    draws = []

    class Counting:
        def randint(self, a, b):
            draws.append((a, b))
            return 5

    items = [case_item(c) for c in bad] + [case_item(good), ((b"\x01" * 47, bytes.fromhex(good["k_r_G"])), 3), (case_item(good)[0], R)]
    prover = P.OpeningBatchProver(device=False)
    out = prover.prove_many(items, rng=Counting())
    assert out[:len(bad)] == [None] * len(bad)
    assert out[len(bad)] is not None
    assert out[len(bad) + 1:] == [None, None]
    assert prover.last_status == [P.BAD_POINT] * len(bad) + [0, 5, P.BAD_SCALAR]     # 5: wrong length (REJECT_LENGTH)
    assert len(draws) == 1                                                            # only the item that decodes draws
    # a blinder of 0 or >= r given by the caller
    proofs, kcs, status = prover.prove_packed(bytes.fromhex(good["r_G"]) + bytes.fromhex(good["k_r_G"]), bytes.fromhex(good["k"]), bytes(32))
    assert status == [P.BAD_BLINDER] and proofs == bytes(128) and kcs == bytes(48)


def test_drop_in_raises_where_reference_raises(P, gold):
    from curdleproofs_pie_amd.shuffle_verifier import is_valid_whisk_opening_proof

    for c in gold["cases"]:
        (r, kr), k = case_item(c)
        if c.get("raises"):
            with pytest.raises(ValueError):
                P.generate_whisk_tracker_proof((r, kr), k)
            continue
        proof = P.generate_whisk_tracker_proof((r, kr), k)
        assert len(proof) == 128
        # a fresh blinder from the global random: other bytes than the fixture's, but a proof the reference's exact check accepts (for a
        # tracker in G1 with k_r_G = k r_G; outside G1, s = b - c k reduced mod r makes the verdict depend on the draw)
        if c["name"] != "k_r_G != k r_G" and "outside G1" not in c["name"]:
            assert is_valid_whisk_opening_proof((r, kr), bytes.fromhex(c["k_commitment"]), proof), c["name"]


def test_seed_derived_blinders_match_hashlib(P, gold):
    seed = bytes(range(32))
    c = gold["cases"][0]
    (r, kr), k = case_item(c)
    n = 5
    trk = (r + kr) * n
    ks = k.to_bytes(32, "little") * n
    proofs, kcs, status = P.OpeningBatchProver(device=False).prove_packed(trk, ks, seed=seed)
    assert status == [0] * n
    for i in range(n):
        b = int.from_bytes(hashlib.shake_256(b"whisk_opening_blinder" + seed + i.to_bytes(8, "little")).digest(64), "little") % R
        assert P.blinders_from_seed(seed, 1, first=i) == b.to_bytes(32, "little")
        gen = c_oracle.scalar_mul(g96(1), b.to_bytes(32, "little"))
        assert proofs[128 * i: 128 * i + 48] == c_oracle.compress(gen)                 # A = b G
        st, rg = c_oracle.decompress(r)
        assert st == 0
        assert proofs[128 * i + 48: 128 * i + 96] == c_oracle.compress(c_oracle.scalar_mul(rg, b.to_bytes(32, "little")))   # B = b r_G
        assert kcs[48 * i: 48 * i + 48] == bytes.fromhex(c["k_commitment"])


def test_generator_multiples_edge_scalars(P):
    rng = random.Random(5)
    ks = [0, 1, 2, R - 1, R - 2, R, R + 1, (R - 1) // 2, 8 * sum(16 ** j for j in range(63)), int("8" * 63, 16), 2 ** 255 - 19, 2 ** 256 - 1]
    ks += [rng.randint(0, 2 ** 256 - 1) for _ in range(6)]
    got = P.generator_multiples(ks, device=False)
    assert got == [O.g1_compress(O.g1_mul(O.G1_GEN, k % R)) for k in ks]
