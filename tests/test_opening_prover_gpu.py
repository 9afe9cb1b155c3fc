"""The opening prover on the GPU (cg1_opening_prove_device, csrc/kernels_opening.h) and the fixed-base kernel of G
(cg1_generator_mul_device, csrc/kernels_generator.h): the reference prover's bytes (tests/golden/opening_prover_vectors.json),
4 096 seeded proofs checked by the batch verifier, by the CPU oracle's group arithmetic and against the host twin, batch-size edges,
bad items, and generator multiples against k_batch_mul and the oracle."""
import ctypes
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

pytestmark = pytest.mark.gpu
R = O.R


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "opening_prover_vectors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def env(native_lib):
    from curdleproofs_pie_amd import opening_prover

    return native_lib, opening_prover, native_lib.default_context()


def g96(k):
    pt = O.g1_mul(O.G1_GEN, k % R)
    return bytes(96) if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def make_items(N, n, seed):
    """n honest trackers (r_G = r G, k_r_G = k r_G) and their k, made with the host pool"""
    rng = random.Random(seed)
    rs = [rng.randint(1, R - 1) for _ in range(n)]
    ks = [rng.randint(1, R - 1) for _ in range(n)]
    rs32 = b"".join(v.to_bytes(32, "little") for v in rs)
    ks32 = b"".join(v.to_bytes(32, "little") for v in ks)
    rG = ctypes.create_string_buffer(96 * n)
    krG = ctypes.create_string_buffer(96 * n)
    assert N.cg1_batch_mul_add_pool(g96(1), 1, rs32, n, None, rG, n, 0) == 0
    assert N.cg1_batch_mul_add_pool(rG.raw, n, ks32, n, None, krG, n, 0) == 0
    trk = b"".join(c_oracle.compress(rG.raw[96 * i: 96 * i + 96]) + c_oracle.compress(krG.raw[96 * i: 96 * i + 96]) for i in range(n))
    return trk, ks32, ks


def test_device_reproduces_fixture(env, gold):
    N, P, ctx = env
    prover = P.OpeningBatchProver(ctx, device=True)
    cases = gold["cases"]
    items = [((bytes.fromhex(c["r_G"]), bytes.fromhex(c["k_r_G"])), int.from_bytes(bytes.fromhex(c["k"]), "little")) for c in cases]
    bl = [int.from_bytes(bytes.fromhex(c["blinder"]), "little") if "blinder" in c else 1 for c in cases]
    out = prover.prove_many(items, blinders=bl)
    for c, o, kc, s in zip(cases, out, prover.last_k_commitments, prover.last_status):
        if c.get("raises"):
            assert o is None and s == P.BAD_POINT, c["name"]
        else:
            assert o == bytes.fromhex(c["proof"]) and kc == bytes.fromhex(c["k_commitment"]), c["name"]


def test_device_seeded_sequence(env, gold):
    N, P, ctx = env
    seq = gold["sequence"]
    items = [((bytes.fromhex(it["r_G"]), bytes.fromhex(it["k_r_G"])), int.from_bytes(bytes.fromhex(it["k"]), "little")) for it in seq["items"]]
    saved = random.getstate()
    try:
        random.seed(seq["seed"])
        got = P.OpeningBatchProver(ctx, device=True).prove_many(items)
        nxt = random.randint(1, R - 1)
    finally:
        random.setstate(saved)
    assert [g.hex() if g is not None else None for g in got] == seq["proofs"]
    assert nxt.to_bytes(32, "little").hex() == seq["next_draw"]


def test_4096_seeded_proofs(env):
    N, P, ctx = env
    from curdleproofs_pie_amd.shuffle_verifier import OpeningBatchVerifier

    n = 4096
    trk, ks32, ks = make_items(N, n, 11)
    seed = hashlib.sha256(b"opening prover test").digest()
    proofs, kcs, status = P.OpeningBatchProver(ctx, device=True).prove_packed(trk, ks32, seed=seed)
    assert status == [0] * n
    # every proof is accepted by the batch verifier (GPU merged check)
    assert all(OpeningBatchVerifier(ctx).verify_packed(trk, kcs, proofs))
    # device == host twin for every item (an extra leg)
    hp, hk, hs = P.OpeningBatchProver(ctx, device=False).prove_packed(trk, ks32, seed=seed)
    assert (hp, hk, hs) == (proofs, kcs, status)
    # 64 items in the CPU oracle's arithmetic: k_G, A, B, and both equalities with c = (b - s) / k
    g = g96(1)
    for i in random.Random(3).sample(range(n), 64):
        k = ks[i]
        b = int.from_bytes(hashlib.shake_256(b"whisk_opening_blinder" + seed + i.to_bytes(8, "little")).digest(64), "little") % R
        st, rG = c_oracle.decompress(trk[96 * i: 96 * i + 48])
        st2, krG = c_oracle.decompress(trk[96 * i + 48: 96 * i + 96])
        assert st == st2 == 0
        pf = proofs[128 * i: 128 * i + 128]
        assert kcs[48 * i: 48 * i + 48] == c_oracle.compress(c_oracle.scalar_mul(g, k.to_bytes(32, "little")))
        assert pf[:48] == c_oracle.compress(c_oracle.scalar_mul(g, b.to_bytes(32, "little")))
        assert pf[48:96] == c_oracle.compress(c_oracle.scalar_mul(rG, b.to_bytes(32, "little")))
        s = int.from_bytes(pf[96:], "little")
        assert s < R
        c = (b - s) * pow(k, -1, R) % R
        sb, cb = s.to_bytes(32, "little"), c.to_bytes(32, "little")
        kG = c_oracle.scalar_mul(g, k.to_bytes(32, "little"))
        assert c_oracle.compress(c_oracle.add(c_oracle.scalar_mul(g, sb), c_oracle.scalar_mul(kG, cb))) == pf[:48]
        assert c_oracle.compress(c_oracle.add(c_oracle.scalar_mul(rG, sb), c_oracle.scalar_mul(krG, cb))) == pf[48:96]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 4160])
def test_batch_sizes_match_host(env, n):
    N, P, ctx = env
    trk, ks32, _ = make_items(N, min(n, 257), 100 + n)
    reps = (n + 256) // 257
    trk, ks32 = (trk * reps)[: 96 * n], (ks32 * reps)[: 32 * n]
    seed = bytes([n % 256]) * 32
    dev = P.OpeningBatchProver(ctx, device=True).prove_packed(trk, ks32, seed=seed)
    host = P.OpeningBatchProver(ctx, device=False).prove_packed(trk, ks32, seed=seed)
    assert dev == host
    assert dev[2] == [0] * n


def test_mixed_bad_items_same_status_as_host(env, gold):
    N, P, ctx = env
    trk, ks32, _ = make_items(N, 96, 7)
    t, k = bytearray(trk), bytearray(ks32)
    bad = [c for c in gold["cases"] if c.get("raises")]
    for j, c in enumerate(bad):                       # bad encodings in r_G / k_r_G
        t[96 * (5 * j): 96 * (5 * j) + 96] = bytes.fromhex(c["r_G"]) + bytes.fromhex(c["k_r_G"])
    k[32 * 3: 32 * 4] = R.to_bytes(32, "little")      # k >= r
    k[32 * 40: 32 * 41] = (2 ** 256 - 1).to_bytes(32, "little")
    bl = bytearray(b"".join(random.Random(9).randint(1, R - 1).to_bytes(32, "little") for _ in range(96)))
    bl[32 * 50: 32 * 51] = bytes(32)                  # blinder 0
    bl[32 * 51: 32 * 52] = R.to_bytes(32, "little")   # blinder >= r
    dev = P.OpeningBatchProver(ctx, device=True).prove_packed(bytes(t), bytes(k), bytes(bl))
    host = P.OpeningBatchProver(ctx, device=False).prove_packed(bytes(t), bytes(k), bytes(bl))
    assert dev == host
    st = dev[2]
    assert [st[5 * j] for j in range(len(bad))] == [P.BAD_POINT] * len(bad)
    assert st[3] == st[40] == P.BAD_SCALAR and st[50] == st[51] == P.BAD_BLINDER
    assert sum(1 for s in st if s) == len(bad) + 4


def test_generator_multiples_vs_batch_mul(env):
    N, P, ctx = env
    n = 1 << 16
    d_sc, d_a, d_b = ctx.alloc(32 * n), ctx.alloc(96 * n), ctx.alloc(96 * n)
    d_g = ctx.alloc(96)
    d_g.upload(g96(1))
    ctx.check(N.cg1_gen_scalars_device(ctx.handle, d_sc.ptr, n, 1234))
    ctx.check(N.cg1_generator_mul_device(ctx.handle, d_sc.ptr, n, d_a.ptr, None))
    ctx.check(N.cg1_batch_mul_device(ctx.handle, d_g.ptr, 1, d_sc.ptr, d_b.ptr, n))
    a, b, sc = d_a.download(96 * n), d_b.download(96 * n), d_sc.download(32 * n)
    assert a == b
    for i in random.Random(4).sample(range(n), 32):
        k = int.from_bytes(sc[32 * i: 32 * i + 32], "little")
        assert a[96 * i: 96 * i + 96] == g96(k)
    rng = random.Random(5)
    ks = [0, 1, 2, R - 1, R - 2, R, R + 1, (R - 1) // 2, 8 * sum(16 ** j for j in range(63)), int("8" * 63, 16), 2 ** 255 - 19, 2 ** 256 - 1]
    ks += [rng.randint(0, 2 ** 256 - 1) for _ in range(100)]
    assert P.generator_multiples(ks, ctx, device=True) == [O.g1_compress(O.g1_mul(O.G1_GEN, v % R)) for v in ks]
    # the raw kernel on unreduced scalars (r, 2 r + 5, values near 2^256: two subtractions of r): the same points as k mod r
    raw = [2 ** 256 - 1, R, 2 * R + 5, 2 ** 256 - 2]
    d_r, d_o = ctx.alloc(32 * len(raw)), ctx.alloc(48 * len(raw))
    d_r.upload(b"".join(v.to_bytes(32, "little") for v in raw))
    ctx.check(N.cg1_generator_mul_device(ctx.handle, d_r.ptr, len(raw), None, d_o.ptr))
    out = d_o.download(48 * len(raw))
    assert [out[48 * i: 48 * i + 48] for i in range(len(raw))] == [O.g1_compress(O.g1_mul(O.G1_GEN, v % R)) for v in raw]
