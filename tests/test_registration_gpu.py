"""Whisk registrations on the GPU (cg1_whisk_register_device, csrc/kernels_register.h): the reference's bytes
(tests/golden/whisk_registration_vectors.json), the host twin at the wave and block edges of the new kernels and on both sides of the size
at which the five multiples change kernels, k_register_points alone against k_generator_mul, an edge grid of scalars against the CPU
oracle's group arithmetic, identity sums inside the shared inversion, refused items, cut invariance, and 4 096 seeded registrations
through the batch verifier, the oracle and the tracker scan."""
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
IDENTITY = b"\xc0" + bytes(47)
G96 = O.G1_GEN[0].to_bytes(48, "little") + O.G1_GEN[1].to_bytes(48, "little")


def le(v):
    return v.to_bytes(32, "little")


def pack(vs):
    return b"".join(le(v) for v in vs)


def g48(v):
    """(v mod r) G compressed, in the CPU oracle's arithmetic"""
    v %= R
    return IDENTITY if v == 0 else c_oracle.compress(c_oracle.scalar_mul(G96, le(v)))


def parts(out, i):
    trk, kcs, pfs, _ = out
    return trk[96 * i: 96 * i + 48], trk[96 * i + 48: 96 * i + 96], kcs[48 * i: 48 * i + 48], pfs[128 * i: 128 * i + 48], pfs[128 * i + 48: 128 * i + 96]


def check_points(out, i, k, r, b, what=""):
    assert parts(out, i) == (g48(r), g48(k * r), g48(k), g48(b), g48(b * r)), (what, i)


def stage(env, cols, shared):
    """the five multiples alone (cg1_whisk_register_points_device): columns [k | b | r | k r | b r] of canonical scalars -> columns
    [k_G | A | r_G | k_r_G | B]; shared: k_register_points (one inversion per item), else k_generator_mul over the 5 n scalars"""
    reg, dev, host, ctx = env
    from curdleproofs_pie_amd import _native as N

    n = len(cols[0])
    assert all(len(c) == n for c in cols) and len(cols) == 5
    d_sc, d_out = ctx.alloc(160 * n), ctx.alloc(240 * n)
    try:
        d_sc.upload(b"".join(pack(c) for c in cols))
        ctx.check(N.cg1_whisk_register_points_device(ctx.handle, d_sc.ptr, n, d_out.ptr, 1 if shared else 0))
        return d_out.download(240 * n)
    finally:
        d_sc.free()
        d_out.free()


def stage_columns(ks, rs, bs):
    return [list(ks), list(bs), list(rs), [k * r % R for k, r in zip(ks, rs)], [b * r % R for b, r in zip(bs, rs)]]


def columns_of(out, n):
    """make_packed's outputs laid out as the stage's columns [k_G | A | r_G | k_r_G | B]"""
    p = [parts(out, i) for i in range(n)]
    return b"".join(b"".join(q[j] for q in p) for j in (2, 3, 0, 1, 4))


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "whisk_registration_vectors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def env(native_lib):
    from curdleproofs_pie_amd import registration

    ctx = native_lib.default_context()
    return registration, registration.RegistrationBatchMaker(ctx, device=True), registration.RegistrationBatchMaker(ctx, device=False), ctx


def test_device_reproduces_fixture(env, gold):
    reg, dev, host, ctx = env
    cases = gold["cases"]
    ks, rs, bs = (b"".join(bytes.fromhex(c[f]) for c in cases) for f in ("k", "r", "b"))
    trk, kcs, pfs, status = dev.make_packed(ks, rs, bs)
    assert status == [0] * len(cases)
    for i, c in enumerate(cases):
        assert trk[96 * i: 96 * i + 96].hex() == c["r_G"] + c["k_r_G"], c["name"]
        assert kcs[48 * i: 48 * i + 48].hex() == c["k_commitment"], c["name"]
        assert pfs[128 * i: 128 * i + 128].hex() == c["proof"], c["name"]


def test_device_reproduces_reference_sequence(env, gold):
    reg, dev, host, ctx = env
    seq = gold["sequence"]
    ks = [int.from_bytes(bytes.fromhex(k), "little") for k in seq["ks"]]
    saved = random.getstate()
    try:
        random.seed(seq["seed"])
        got = dev.make_many(ks)
        nxt = random.randint(1, R - 1)
    finally:
        random.setstate(saved)
    assert dev.last_status == [0] * len(ks)
    for g, it in zip(got, seq["items"]):
        (r_G, k_r_G), kc, proof = g
        assert (r_G.hex(), k_r_G.hex(), kc.hex(), proof.hex()) == (it["r_G"], it["k_r_G"], it["k_commitment"], it["proof"])
    assert le(nxt).hex() == seq["next_draw"]


# 32 768 / 32 769: the last size whose five multiples go through k_generator_mul and the first that takes k_register_points
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025, 32768, 32769])
def test_sizes_match_host_twin(env, n):
    reg, dev, host, ctx = env
    rng = random.Random(1000 + n)
    ks32 = pack(rng.randint(0, R - 1) for _ in range(n))
    seed = hashlib.sha256(b"registration sizes %d" % n).digest()
    d = dev.make_packed(ks32, seed=seed, first_index=n)
    assert d == host.make_packed(ks32, seed=seed, first_index=n)
    assert d[3] == [0] * n


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025, 131072 + 257])
def test_shared_inversion_kernel_at_its_edges(env, n):
    """k_register_points alone at the wave and block edges and past one item per lane of its largest grid (131 072 lanes: the lanes
    then take a second item): the bytes of k_generator_mul over the same 5 n scalars, zero scalars (identity sums) scattered through
    every column, and the oracle's points for a sample"""
    rng = random.Random(2000 + n)
    cols = [[rng.randint(0, R - 1) if rng.random() > 0.05 else 0 for _ in range(n)] for _ in range(5)]
    if n >= 64:
        for j in range(5):
            cols[j][63 - j] = EDGES[j + 5]
        cols = [[0 if i == 17 else v for i, v in enumerate(c)] for c in cols]                # a lane whose five sums are all the identity
    got = stage(env, cols, True)
    assert got == stage(env, cols, False)
    for i in sorted(set(random.Random(n).sample(range(n), min(n, 12))) | ({17, 59, 63} if n >= 64 else set())):
        for j in range(5):
            assert got[48 * (j * n + i): 48 * (j * n + i) + 48] == g48(cols[j][i]), (n, i, j)


# values that drive the carries of the signed 8-bit recoding (a byte of 0x80 is the first to borrow from the window above, a run of
# them carries through every window) and the reductions of the Fr products k r and b r
EDGES = [1, 2, 127, 128, 129, 255, 256, int.from_bytes(b"\x80" * 32, "little") % R, int.from_bytes(b"\x7f" * 32, "little") % R, R - 1, R - 2, pow(2, 255, R)]


def test_edge_grid_against_the_oracle(env):
    reg, dev, host, ctx = env
    items = [(k, r, EDGES[(i + j) % len(EDGES)]) for i, k in enumerate(EDGES) for j, r in enumerate(EDGES)]        # every pair (k, r), b cycling
    assert {b for _, _, b in items} == set(EDGES)
    out = dev.make_packed(pack(k for k, _, _ in items), pack(r for _, r, _ in items), pack(b for _, _, b in items))
    assert out[3] == [0] * len(items)
    for i, (k, r, b) in enumerate(items):
        check_points(out, i, k, r, b, "edge grid")
    cols = stage_columns(*zip(*[(k, r, b) for k, r, b in items]))
    assert stage(env, cols, True) == columns_of(out, len(items))              # the same grid through k_register_points
    assert out == host.make_packed(pack(k for k, _, _ in items), pack(r for _, r, _ in items), pack(b for _, _, b in items))


def test_identity_sums_inside_the_shared_inversion(env):
    reg, dev, host, ctx = env
    rng = random.Random(5)
    n = 64
    ks, rs, bs = ([rng.randint(1, R - 1) for _ in range(n)] for _ in range(3))
    base = dev.make_packed(pack(ks), pack(rs), pack(bs))
    zeros = (0, 1, 31, 32, 62, 63, 17)
    kz = [0 if i in zeros else k for i, k in enumerate(ks)]
    out = dev.make_packed(pack(kz), pack(rs), pack(bs))
    assert out[3] == [0] * n
    for i in range(n):
        if i in zeros:
            r_G, k_r_G, k_G, A, B = parts(out, i)
            assert k_r_G == IDENTITY and k_G == IDENTITY
            assert (r_G, A, B) == (g48(rs[i]), g48(bs[i]), g48(bs[i] * rs[i]))
            assert out[2][128 * i + 96: 128 * i + 128] == le(bs[i])          # s = b - c 0
        else:                                                                 # the neighbours: what they are without the zeros
            assert parts(out, i) == parts(base, i) and out[2][128 * i: 128 * i + 128] == base[2][128 * i: 128 * i + 128]
    whole = dev.make_packed(bytes(32 * n), pack(rs), pack(bs))
    assert whole[3] == [0] * n
    for i in range(n):
        assert parts(whole, i) == (g48(rs[i]), IDENTITY, IDENTITY, g48(bs[i]), g48(bs[i] * rs[i]))
    assert whole == host.make_packed(bytes(32 * n), pack(rs), pack(bs)) and out == host.make_packed(pack(kz), pack(rs), pack(bs))
    # the same three batches through k_register_points, whose product chain the identity sums must stay out of
    for kk, want in ((ks, base), (kz, out), ([0] * n, whole)):
        assert stage(env, stage_columns(kk, rs, bs), True) == columns_of(want, n)


BAD = [("k", R, 1), ("k", 2 ** 256 - 1, 1), ("r", 0, 4), ("r", R, 4), ("b", 0, 4), ("b", R, 4)]


def test_mixed_bad_items(env):
    reg, dev, host, ctx = env
    rng = random.Random(6)
    n, where = 102, (0, 17, 63, 64, 65, 101)
    cols = {f: [rng.randint(1, R - 1) for _ in range(n)] for f in ("k", "r", "b")}
    good = {f: [v for i, v in enumerate(cols[f]) if i not in where] for f in cols}
    for (field, value, _), i in zip(BAD, where):
        cols[field][i] = value
    out = dev.make_packed(*(b"".join(v.to_bytes(32, "little") for v in cols[f]) for f in ("k", "r", "b")))
    assert out == host.make_packed(*(b"".join(v.to_bytes(32, "little") for v in cols[f]) for f in ("k", "r", "b")))
    want = [0] * n
    for (_, _, code), i in zip(BAD, where):
        want[i] = code
    assert out[3] == want and (reg.BAD_SCALAR, reg.BAD_BLINDER) == (1, 4)
    for i in where:
        assert out[0][96 * i: 96 * i + 96] == bytes(96) and out[1][48 * i: 48 * i + 48] == bytes(48) and out[2][128 * i: 128 * i + 128] == bytes(128)
    alone = dev.make_packed(pack(good["k"]), pack(good["r"]), pack(good["b"]))            # the 96 good ones without the refused
    assert alone[3] == [0] * 96
    j = 0
    for i in range(n):
        if i in where:
            continue
        assert parts(out, i) == parts(alone, j) and out[2][128 * i: 128 * i + 128] == alone[2][128 * j: 128 * j + 128]
        j += 1


def test_cut_invariance(env):
    reg, dev, host, ctx = env
    rng = random.Random(8)
    n, h = 300, 77
    ks32 = pack(rng.randint(0, R - 1) for _ in range(n))
    seed = hashlib.sha256(b"registration cut").digest()
    whole = dev.make_packed(ks32, seed=seed, first_index=5)
    head, tail = dev.make_packed(ks32[: 32 * h], seed=seed, first_index=5), dev.make_packed(ks32[32 * h:], seed=seed, first_index=5 + h)
    assert tuple(a + b for a, b in zip(head, tail)) == whole
    assert dev.make_packed(ks32, seed=seed, first_index=5) == whole
    assert reg.RegistrationBatchMaker(ctx, device=True, max_items=128).make_packed(ks32, seed=seed, first_index=5) == whole
    assert dev.make_packed(ks32, seed=seed, first_index=6) != whole


def test_4096_seeded_registrations_round_trip(env):
    reg, dev, host, ctx = env
    from curdleproofs_pie_amd.shuffle_verifier import OpeningBatchVerifier
    from curdleproofs_pie_amd.tracker_scan import TrackerScanner

    n = 4096
    rng = random.Random(12)
    ks = [rng.randint(1, R - 1) for _ in range(n)]
    seed = hashlib.sha256(b"registration round trip").digest()
    out = dev.make_packed(pack(ks), seed=seed)
    trk, kcs, pfs, status = out
    assert status == [0] * n
    assert all(OpeningBatchVerifier(ctx).verify_packed(trk, kcs, pfs))
    sample = random.Random(3).sample(range(n), 64)
    for i in sample:
        k = ks[i]
        r, b = (int.from_bytes(hashlib.shake_256(b"whisk_registration_draw" + seed + i.to_bytes(8, "little") + d.to_bytes(4, "little")).digest(64), "little") % R
                for d in (0, 1))
        check_points(out, i, k, r, b, "round trip")
        s = int.from_bytes(pfs[128 * i + 96: 128 * i + 128], "little")
        assert s < R
        c = (b - s) * pow(k, -1, R) % R
        rG, krG, kG = (c_oracle.scalar_mul(G96, le(v % R)) for v in (r, k * r, k))
        assert c_oracle.compress(c_oracle.add(c_oracle.scalar_mul(G96, le(s)), c_oracle.scalar_mul(kG, le(c)))) == pfs[128 * i: 128 * i + 48]
        assert c_oracle.compress(c_oracle.add(c_oracle.scalar_mul(rG, le(s)), c_oracle.scalar_mul(krG, le(c)))) == pfs[128 * i + 48: 128 * i + 96]
    bitmap, tstat, kstat = TrackerScanner(ctx, device=True).scan_packed(b"".join(trk[96 * i: 96 * i + 96] for i in sample), pack(ks[i] for i in sample))
    assert tstat == [0] * 64 and kstat == [0] * 64
    assert bitmap == b"".join((1 << j).to_bytes(8, "little") for j in range(64))
