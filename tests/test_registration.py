"""Whisk registrations made in bulk (curdleproofs_pie_amd.registration) on the host twin (cg1_whisk_register): the reference's bytes for
generate_tracker + get_k_commitment + GenerateWhiskTrackerProof (tests/golden/whisk_registration_vectors.json), its draw sequence under one
random.seed, the seed derivation in its three copies (hashlib, the host's C, the fixture), status codes and zeroed outputs of refused
items, and the argument checks."""
import ctypes
import hashlib
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
IDENTITY = b"\xc0" + bytes(47)


def le(v):
    return v.to_bytes(32, "little")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "whisk_registration_vectors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def reg(native_lib):
    from curdleproofs_pie_amd import registration

    return registration


def test_host_twin_reproduces_fixture(reg, gold):
    cases = gold["cases"]
    ks, rs, bs = (b"".join(bytes.fromhex(c[f]) for c in cases) for f in ("k", "r", "b"))
    trk, kcs, pfs, status = reg.RegistrationBatchMaker(device=False).make_packed(ks, rs, bs)
    assert status == [0] * len(cases)
    for i, c in enumerate(cases):
        assert trk[96 * i: 96 * i + 96].hex() == c["r_G"] + c["k_r_G"], c["name"]
        assert kcs[48 * i: 48 * i + 48].hex() == c["k_commitment"], c["name"]
        assert pfs[128 * i: 128 * i + 128].hex() == c["proof"], c["name"]
    by_name = {c["name"]: c for c in cases}
    assert bytes.fromhex(by_name["k = 0"]["k_r_G"]) == IDENTITY and bytes.fromhex(by_name["k = 0"]["k_commitment"]) == IDENTITY
    assert by_name["k = 1 / r (k_r_G = G)"]["k_r_G"] == by_name["k = 1"]["k_commitment"]       # both are G


def test_make_many_reproduces_reference_sequence(reg, gold):
    seq = gold["sequence"]
    ks = [int.from_bytes(bytes.fromhex(k), "little") for k in seq["ks"]]
    maker = reg.RegistrationBatchMaker(device=False)
    saved = random.getstate()
    try:
        random.seed(seq["seed"])
        got = maker.make_many(ks)
        nxt = random.randint(1, R - 1)
    finally:
        random.setstate(saved)
    assert maker.last_status == [0] * len(ks)
    for g, it in zip(got, seq["items"]):
        (r_G, k_r_G), kc, proof = g
        assert (r_G.hex(), k_r_G.hex(), kc.hex(), proof.hex()) == (it["r_G"], it["k_r_G"], it["k_commitment"], it["proof"])
    assert le(nxt).hex() == seq["next_draw"]
    # an rng of the caller's, and a k the native code refuses: no draw for it, None in its place
    rng = random.Random(seq["seed"])
    got2 = maker.make_many(ks[:3] + [R] + ks[3:6], rng=rng)
    assert got2[3] is None and maker.last_status == [0, 0, 0, reg.BAD_SCALAR, 0, 0, 0]
    assert got2[:3] + got2[4:] == got[:6]


def test_draws_three_copies_agree(reg, gold, native_lib):
    N = native_lib
    seed = bytes.fromhex(gold["seeded"]["seed"])
    for d in gold["seeded"]["draws"]:
        r, b = reg.registration_draws_from_seed(seed, d["index"])
        assert (le(r).hex(), le(b).hex()) == (d["r"], d["b"])
        o_r, o_b = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        assert N.cg1_whisk_register_draws(seed, d["index"], 1, o_r, o_b) == 0
        assert (o_r.raw.hex(), o_b.raw.hex()) == (d["r"], d["b"])
    n, first = 70, 250
    o_r, o_b = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n)
    assert N.cg1_whisk_register_draws(seed, first, n, o_r, o_b) == 0
    want = [reg.registration_draws_from_seed(seed, first + i) for i in range(n)]
    assert o_r.raw == b"".join(le(r) for r, _ in want) and o_b.raw == b"".join(le(b) for _, b in want)
    assert N.cg1_whisk_register_draws(seed, (1 << 32) - 1, 2, o_r, o_b) == 1           # CG1_ERR_ARG: an index past 2^32 - 1
    with pytest.raises(ValueError):
        reg.registration_draws_from_seed(seed[:31], 0)
    with pytest.raises(ValueError):
        reg.registration_draws_from_seed(seed, 1 << 32)


def test_seeded_host_twin_uses_the_derivation(reg, gold):
    """make_packed(seed) on the host == make_packed with the hashlib draws supplied; cutting a batch changes nothing"""
    seed = hashlib.sha256(b"registration host test").digest()
    rng = random.Random(1)
    ks = [rng.randint(0, R - 1) for _ in range(21)]
    ks32 = b"".join(le(k) for k in ks)
    maker = reg.RegistrationBatchMaker(device=False)
    whole = maker.make_packed(ks32, seed=seed, first_index=1000)
    draws = [reg.registration_draws_from_seed(seed, 1000 + i) for i in range(21)]
    assert whole == maker.make_packed(ks32, b"".join(le(r) for r, _ in draws), b"".join(le(b) for _, b in draws))
    head, tail = maker.make_packed(ks32[: 32 * 8], seed=seed, first_index=1000), maker.make_packed(ks32[32 * 8:], seed=seed, first_index=1008)
    assert tuple(h + t for h, t in zip(head, tail)) == whole
    cut = reg.RegistrationBatchMaker(device=False, max_items=5).make_packed(ks32, seed=seed, first_index=1000)
    assert cut == whole


BAD = [("k", R, "BAD_SCALAR"), ("k", 2 ** 256 - 1, "BAD_SCALAR"), ("r", 0, "BAD_BLINDER"), ("r", R, "BAD_BLINDER"), ("b", 0, "BAD_BLINDER"),
       ("b", R, "BAD_BLINDER")]


def mixed_inputs(n=20, where=(2, 5, 6, 11, 12, 19)):
    rng = random.Random(77)
    cols = {f: [rng.randint(1, R - 1) for _ in range(n)] for f in ("k", "r", "b")}
    for (field, value, _), i in zip(BAD, where):
        cols[field][i] = value
    return tuple(b"".join(le(v) for v in cols[f]) for f in ("k", "r", "b")), where


def test_refused_items_get_codes_and_zeros(reg):
    (ks, rs, bs), where = mixed_inputs()
    n = len(ks) // 32
    maker = reg.RegistrationBatchMaker(device=False)
    trk, kcs, pfs, status = maker.make_packed(ks, rs, bs)
    want = [0] * n
    for (_, _, code), i in zip(BAD, where):
        want[i] = getattr(reg, code)
    assert status == want and (reg.BAD_SCALAR, reg.BAD_BLINDER) == (1, 4)
    # the neighbours are what they are alone
    good = [i for i in range(n) if not want[i]]
    alone = maker.make_packed(*(b"".join(col[32 * i: 32 * i + 32] for i in good) for col in (ks, rs, bs)))
    assert alone[3] == [0] * len(good)
    for j, i in enumerate(good):
        assert trk[96 * i: 96 * i + 96] == alone[0][96 * j: 96 * j + 96] and kcs[48 * i: 48 * i + 48] == alone[1][48 * j: 48 * j + 48]
        assert pfs[128 * i: 128 * i + 128] == alone[2][128 * j: 128 * j + 128]
    for i in where:
        assert trk[96 * i: 96 * i + 96] == bytes(96) and kcs[48 * i: 48 * i + 48] == bytes(48) and pfs[128 * i: 128 * i + 128] == bytes(128)


def test_argument_checks(reg, native_lib):
    N = native_lib
    maker = reg.RegistrationBatchMaker(device=False)
    assert maker.make_packed(b"") == (b"", b"", b"", []) and maker.make_many([]) == []
    assert maker.make_packed(b"", b"", b"") == (b"", b"", b"", [])
    k = le(5)
    for args in ((k[:31],), (k + b"\0",), (k, k), (k, None, k), (k, k + k, k), (k, k, k[:16])):
        with pytest.raises(ValueError):
            maker.make_packed(*args)
    with pytest.raises(ValueError):
        maker.make_packed(k, seed=bytes(31))
    with pytest.raises(ValueError):
        maker.make_packed(k + k, seed=bytes(32), first_index=(1 << 32) - 1)
    with pytest.raises(ValueError):
        maker.make_many([1 << 256])
    with pytest.raises(ValueError):
        reg.make_whisk_registration(R)
    # the native refusals come before anything is written
    out = [ctypes.create_string_buffer(b"\xaa" * s, s) for s in (96, 48, 128)]
    st = (ctypes.c_int32 * 1)(7)
    assert N.cg1_whisk_register(1, k, k, None, out[0], out[1], out[2], st) != 0
    assert N.cg1_whisk_register(1, k, None, None, out[0], out[1], out[2], st) != 0
    assert N.cg1_whisk_register(1 << 26, k, k, k, out[0], out[1], out[2], st) != 0
    assert [o.raw for o in out] == [b"\xaa" * s for s in (96, 48, 128)] and st[0] == 7


def test_one_use_functions_verify(reg, native_lib):
    """fresh seeds: two calls differ, and each registration passes the host's exact opening check (both verifier equalities)"""
    (r_G, k_r_G), kc, proof = reg.make_whisk_registration(12345)
    again = reg.make_whisk_registration(12345)
    assert again[1] == kc and again[0] != (r_G, k_r_G)
    many = reg.make_whisk_registrations([0, 1, R - 1, R], device=False)
    assert many[3] is None and all(m is not None for m in many[:3])
    for (t0, t1), c, p in [((r_G, k_r_G), kc, proof)] + many[:3]:
        ok = ctypes.c_int(0)
        assert native_lib.cg1_opening_exact(t0 + t1, c, p, ctypes.byref(ok)) == 0 and ok.value == 1
