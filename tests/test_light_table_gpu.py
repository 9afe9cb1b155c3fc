"""Light tables and k_table_msm's light plan (csrc/kernels_light.h) against the CPU oracle, bit for bit.  Needs an MI355X.

Every expected value comes from the oracle (C.msm_bucket / O.g1_mul / O.g1_add), never from another path of the product -- except the
last two tests, which are about the two table classes agreeing and about the recorded rounds of the reference prover.  The tables are built once per module: 40 oracle-made points, and a 12-base table of
special points (the identity, equal points, the order-3 point, a point outside G1, the generator)."""
import ctypes
import json
import os
import random
import sys

import pytest

from conftest import raw96
from oracle import bls12_381 as O
from oracle import c_oracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
NEG = 1 << 31


@pytest.fixture(scope="module")
def ctx(native_lib):
    c = native_lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pts40():
    rng = random.Random(4000)
    return [O.g1_mul(O.G1_GEN, rng.randint(1, O.R - 1)) for _ in range(40)]


@pytest.fixture(scope="module")
def tab40(native_lib, ctx, pts40):
    c = native_lib.LIGHT_WINDOW_BITS
    t = ctx.light_table(b"".join(raw96(p) for p in pts40), 40)
    assert t.nbytes == 40 * ((256 + c - 1) // c) * (1 << (c - 1)) * 256
    assert native_lib.cg1_light_len(t.handle) == 40
    yield t
    t.free()


@pytest.fixture(scope="module")
def special(ctx, pts40):
    tors = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_vectors.json")))
    T3 = O.g1_decompress(bytes.fromhex(tors["t3"]))
    assert T3 == (0, 2) and O.g1_is_on_curve(T3) and not O.g1_in_subgroup(T3) and O.g1_mul(T3, 3) is None
    mixed = O.g1_add(T3, pts40[9])                                       # order 3 r: outside G1, not of small order
    # 0: identity   1, 2: equal points   3: T3   4: T3 + P   5: the generator   6 ..: ordinary points
    pts = [None, pts40[0], pts40[0], T3, mixed, O.G1_GEN] + pts40[1:7]
    tab = ctx.light_table(b"".join(raw96(p) for p in pts), len(pts))
    yield tab, pts, T3, mixed
    tab.free()


def s32(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def neg(pt):
    return None if pt is None else (pt[0], (O.P - pt[1]) % O.P)


def want48(pts, idx, sc):
    """The oracle's compressed sum of sc[i] * pts[idx[i]] (bit 31 of an index = the negated base)."""
    p96 = b"".join(raw96(neg(pts[i & ~NEG]) if i & NEG else pts[i]) for i in idx)
    return C.compress(C.msm_bucket(p96, s32(sc), len(idx))) if idx else O.g1_compress(None)


def want48_any(pts, idx, sc):
    """The same through the oracle's double-and-add, which takes the INTEGER scalar as it is: for bases outside G1."""
    acc = None
    for i, v in zip(idx, sc):
        b = pts[i & ~NEG]
        acc = O.g1_add(acc, O.g1_mul(neg(b) if i & NEG else b, v))
    return O.g1_compress(acc)


def got48(ctx, tab, idx, sc, offsets=None):
    offsets = [0, len(idx)] if offsets is None else offsets
    out = ctx.light_msm_host(tab, idx, s32(sc), offsets, compressed=True)
    return out[0] if len(offsets) == 2 else out


def test_every_term_count(native_lib, ctx, tab40, pts40):
    """1 .. 130 terms, each count an MSM of ONE call (so every launch shape from one term per workgroup upwards is taken by some call:
    the counts are also run one per call in groups below)."""
    rng = random.Random(4001)
    idx, sc, offsets = [], [], [0]
    for n in range(1, 131):
        idx += [rng.randrange(40) for _ in range(n)]
        sc += [rng.randrange(O.R) for _ in range(n)]
        offsets.append(len(idx))
    got = ctx.light_msm_host(tab40, idx, s32(sc), offsets, compressed=True)
    for j, n in enumerate(range(1, 131)):
        a, b = offsets[j], offsets[j + 1]
        assert got[j] == want48(pts40, idx[a:b], sc[a:b]), n
    for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, 130):                   # alone in a call: the slice is sized by this count
        a, b = offsets[n - 1], offsets[n]
        assert got48(ctx, tab40, idx[a:b], sc[a:b]) == got[n - 1], n
    # the blob output is the same point
    blob = ctx.light_msm_host(tab40, [5, 7, 5], s32([3, 4, O.R - 2]), [0, 3])[0]
    out = ctypes.create_string_buffer(48)
    native_lib.cg1_compress(out, blob)
    assert out.raw == want48(pts40, [5, 7, 5], [3, 4, O.R - 2])


def test_slice_join_up_to_the_limit(native_lib, ctx, tab40, pts40):
    """Counts that take several workgroups per MSM (the ticketed join), the per-MSM limit included, alone and beside short MSMs."""
    N = native_lib
    rng = random.Random(4002)
    for n in (300, 1024, N.LIGHT_MAX_TERMS):
        idx = [rng.randrange(40) | (NEG if rng.random() < 0.2 else 0) for _ in range(n)]
        sc = [rng.randrange(O.R) for _ in range(n)]
        assert got48(ctx, tab40, idx, sc) == want48(pts40, idx, sc), n
    ctx.set_param("fixed_slice", 4)                                       # many slices of a short MSM: 65 terms = 17 workgroups
    try:
        idx = [rng.randrange(40) for _ in range(65)]
        sc = [rng.randrange(O.R) for _ in range(65)]
        assert got48(ctx, tab40, idx + [3], sc + [9], [0, 65, 65, 66]) == [want48(pts40, idx, sc), O.g1_compress(None), want48(pts40, [3], [9])]
    finally:
        ctx.set_param("fixed_slice", 0)
    with pytest.raises(N.NativeError):
        ctx.light_msm_host(tab40, [0] * (N.LIGHT_MAX_TERMS + 1), s32([1] * (N.LIGHT_MAX_TERMS + 1)), [0, N.LIGHT_MAX_TERMS + 1])
    with pytest.raises(N.NativeError):
        ctx.light_msm_host(tab40, [], b"", [0] * (N.LIGHT_MAX_MSMS + 2))


@pytest.mark.parametrize("m", [1, 7, 64, 256])
def test_uneven_batches(ctx, tab40, pts40, m):
    rng = random.Random(4003 + m)
    lens = [rng.choice([0, 0, 1, 2, 7, 8, 9, 15, 16, 17, 33, 64, 64, 65, 128, 200]) for _ in range(m)]
    if m >= 4:
        lens[0], lens[-1], lens[m // 2] = 0, 0, 500                      # empty MSMs at both ends, one far longer than the rest
    idx, sc, offsets = [], [], [0]
    for n in lens:
        idx += [rng.randrange(40) | (NEG if rng.random() < 0.2 else 0) for _ in range(n)]
        sc += [rng.randrange(O.R) for _ in range(n)]
        offsets.append(len(idx))
    got = ctx.light_msm_host(tab40, idx, s32(sc), offsets, compressed=True)
    assert len(got) == m
    for j in range(m):
        a, b = offsets[j], offsets[j + 1]
        assert got[j] == want48(pts40, idx[a:b], sc[a:b]), (m, j, lens[j])


def test_scalars_and_indices(native_lib, ctx, tab40, pts40):
    rng = random.Random(4004)
    k = rng.randrange(O.R)
    for n in (1, 40, 64):
        idx = [i % 40 for i in range(n)]
        for name, sc in (("equal", [k] * n), ("small", list(range(n))), ("r-1", [O.R - 1] * n), ("zeros", [0] * n), ("ones", [1] * n),
                         ("one hot", [0] * (n - 1) + [k]), ("2^k", [1 << (i * 4 % 255) for i in range(n)])):
            assert got48(ctx, tab40, idx, sc) == want48(pts40, idx, sc), (name, n)
    assert got48(ctx, tab40, [3] * 4, [0] * 4) == O.g1_compress(None)
    for n in (2, 40, 300):                                                # the same index many times
        sc = [rng.randrange(O.R) for _ in range(n)]
        assert got48(ctx, tab40, [6] * n, sc) == O.g1_compress(O.g1_mul(pts40[6], sum(sc) % O.R)), n
        assert got48(ctx, tab40, [6] * n, [k] * n) == O.g1_compress(O.g1_mul(pts40[6], k * n % O.R)), n
    assert got48(ctx, tab40, [7, 7 | NEG], [k, k]) == O.g1_compress(None)                    # k B + k (-B)
    assert got48(ctx, tab40, [7, 8, 7 | NEG], [k, 3, k]) == O.g1_compress(O.g1_mul(pts40[8], 3))
    assert got48(ctx, tab40, [7 | NEG], [k]) == O.g1_compress(O.g1_mul(neg(pts40[7]), k))


def test_special_bases(native_lib, ctx, special):
    tab, pts, T3, mixed = special
    rng = random.Random(4005)
    k = rng.randrange(O.R)
    assert got48(ctx, tab, [0], [k]) == O.g1_compress(None)                                  # the identity base
    assert got48(ctx, tab, [0, 6, 0], [k, 7, 1]) == want48(pts, [0, 6, 0], [k, 7, 1])
    assert got48(ctx, tab, [1, 2], [k, k]) == O.g1_compress(O.g1_mul(pts[1], 2 * k % O.R))   # two table bases that are equal points: P + P
    assert got48(ctx, tab, [1, 2 | NEG], [k, k]) == O.g1_compress(None)
    assert got48(ctx, tab, [5], [k]) == O.g1_compress(O.g1_mul(O.G1_GEN, k))
    # bases outside G1: k P depends on the INTEGER k.  Every digit value of window 0 and 1, both signs, and full-width scalars
    ks = list(range(1, 40)) + [255, 256, 257, O.R - 1, O.R - 2, k] + [rng.randrange(O.R) for _ in range(6)]
    idx, sc, offsets = [], [], [0]
    for kk in ks:
        for b in (3, 4, 3 | NEG):
            idx.append(b); sc.append(kk); offsets.append(len(idx))
    got = ctx.light_msm_host(tab, idx, s32(sc), offsets, compressed=True)
    for j, (i, kk) in enumerate(zip(idx, sc)):
        assert got[j] == want48_any(pts, [i], [kk]), (i & ~NEG, kk)
    assert O.g1_mul(T3, O.R - 1) is None and O.g1_mul(T3, O.R - 2) is not None              # r = 1 (mod 3): the integer matters
    sc = [rng.randrange(O.R) for _ in range(7)]
    idx = [3, 4, 6, 3 | NEG, 4, 7, 0]
    assert got48(ctx, tab, idx, sc) == want48_any(pts, idx, sc)


def test_device_entry_equals_host_entry(native_lib, ctx, tab40, pts40):
    rng = random.Random(4006)
    lens = [0, 1, 64, 64, 9, 0, 300, 40, 16, 17, 3]
    idx, sc, offsets = [], [], [0]
    for n in lens:
        idx += [rng.randrange(40) | (NEG if rng.random() < 0.3 else 0) for _ in range(n)]
        sc += [rng.randrange(O.R) for _ in range(n)]
        offsets.append(len(idx))
    m, nt = len(lens), len(idx)
    host = ctx.light_msm_host(tab40, idx, s32(sc), offsets, compressed=True)
    for j in range(m):
        assert host[j] == want48(pts40, idx[offsets[j]:offsets[j + 1]], sc[offsets[j]:offsets[j + 1]]), j
    d_tb, d_sc, d_off = ctx.alloc(4 * nt), ctx.alloc(32 * nt), ctx.alloc(4 * (m + 1))
    d_a, d_k = ctx.alloc(96 * m), ctx.alloc(48 * m)
    d_tb.upload(b"".join(i.to_bytes(4, "little") for i in idx)); d_sc.upload(s32(sc)); d_off.upload(b"".join(o.to_bytes(4, "little") for o in offsets))
    try:
        for outs in ((d_a, d_k), (d_a, None), (None, d_k)):
            d_a.upload(b"\x55" * (96 * m)); d_k.upload(b"\x55" * (48 * m))
            ctx.light_msm_device(tab40, d_tb, d_sc, d_off, m, nt, max(lens), outs[0], outs[1])
            if outs[1] is not None:
                k48 = d_k.download()
                assert [k48[48 * j: 48 * j + 48] for j in range(m)] == host
            if outs[0] is not None:
                a96 = d_a.download()
                for j in range(m):
                    assert C.compress(a96[96 * j: 96 * j + 96]) == host[j], j
        # a scalar >= r, then an index outside the table, among the device arrays: the documented errors, outputs untouched
        bad = list(sc); bad[70] = O.R
        d_sc.upload(s32(bad))
        d_a.upload(b"\x55" * (96 * m)); d_k.upload(b"\x55" * (48 * m))
        with pytest.raises(native_lib.NativeError):
            ctx.light_msm_device(tab40, d_tb, d_sc, d_off, m, nt, max(lens), d_a, d_k)
        assert d_a.download() == b"\x55" * (96 * m) and d_k.download() == b"\x55" * (48 * m)
        d_sc.upload(s32(sc))
        bad_idx = list(idx); bad_idx[5] = 40
        d_tb.upload(b"".join(i.to_bytes(4, "little") for i in bad_idx))
        with pytest.raises(native_lib.NativeError):
            ctx.light_msm_device(tab40, d_tb, d_sc, d_off, m, nt, max(lens), d_a, d_k)
        assert d_a.download() == b"\x55" * (96 * m) and d_k.download() == b"\x55" * (48 * m)
        d_tb.upload(b"".join(i.to_bytes(4, "little") for i in idx))
        ctx.light_msm_device(tab40, d_tb, d_sc, d_off, m, nt, max(lens), None, d_k)          # and the table works on
        k48 = d_k.download()
        assert [k48[48 * j: 48 * j + 48] for j in range(m)] == host
    finally:
        for b in (d_tb, d_sc, d_off, d_a, d_k):
            b.free()


def test_refusals_write_nothing(native_lib, ctx, tab40, pts40):
    N = native_lib
    for bad_sc, bad_idx, rc in ((O.R, 3, N.ERR_ENCODING), (O.R + 1, 3, N.ERR_ENCODING), ((1 << 256) - 1, 3, N.ERR_ENCODING), (6, 40, N.ERR_ARG),
                                (6, 40 | NEG, N.ERR_ARG)):
        idx, sc, offsets = [1, 2, bad_idx, 4], [5, 6, bad_sc, 7], [0, 2, 4]
        tb = (ctypes.c_uint32 * 4)(*idx)
        offs = (ctypes.c_uint32 * 3)(*offsets)
        blobs = ctypes.create_string_buffer(b"\xaa" * (2 * N.POINT_BYTES), 2 * N.POINT_BYTES)
        comp = ctypes.create_string_buffer(b"\xaa" * 96, 96)
        assert N.cg1_light_msm(ctx.handle, tab40.handle, tb, s32(sc), offs, 2, blobs, comp) == rc
        assert blobs.raw == b"\xaa" * (2 * N.POINT_BYTES) and comp.raw == b"\xaa" * 96
    assert got48(ctx, tab40, [1, 2], [5, 6]) == want48(pts40, [1, 2], [5, 6])                # the table works on after a refused call
    st = ctypes.c_int(0)
    assert not N.cg1_light_create(ctx.handle, bytes(96), N.LIGHT_MAX_BASES + 1, ctypes.byref(st)) and st.value == N.ERR_ARG
    assert not N.cg1_light_create(ctx.handle, bytes(96), 0, ctypes.byref(st)) and st.value == N.ERR_ARG
    bad = (O.P).to_bytes(48, "little") + (2).to_bytes(48, "little")                          # x = p: not canonical
    assert not N.cg1_light_create(ctx.handle, bad, 1, ctypes.byref(st)) and st.value == N.ERR_ENCODING
    off = (1).to_bytes(48, "little") + (1).to_bytes(48, "little")                            # 1 != 1 + 4: off the curve
    assert not N.cg1_light_create(ctx.handle, off, 1, ctypes.byref(st)) and st.value == N.ERR_NOT_ON_CURVE


def test_fixed_and_light_tables_alternate_on_one_context(ctx, pts40):
    """The two kinds share one kernel and one host layer: the context's sequence number and flag wait, and each handle's OWN ticket
    words and staging block.  Host entries on a fixed and a light table over the same 8 points, turn and turn about -- 3 MSMs of 1, 5
    and 0 terms -- first at the calls' own shape, then with 2 terms per workgroup (the 5-term MSM goes through the ticketed join)."""
    pts = pts40[:8]
    raw = b"".join(raw96(p) for p in pts)
    fixed, light = ctx.fixed_table(raw, 8), ctx.light_table(raw, 8)
    rng = random.Random(4008)
    try:
        for fixed_slice in (0, 2):
            ctx.set_param("fixed_slice", fixed_slice)
            for turn in range(4):
                for kind, entry, tab in (("fixed", ctx.fixed_msm_host, fixed), ("light", ctx.light_msm_host, light)):
                    idx = [rng.randrange(8) | (NEG if rng.random() < 0.3 else 0) for _ in range(6)]
                    sc = [rng.randrange(O.R) for _ in range(6)]
                    got = entry(tab, idx, s32(sc), [0, 1, 6, 6], compressed=True)
                    assert got == [want48(pts, idx[:1], sc[:1]), want48(pts, idx[1:], sc[1:]), O.g1_compress(None)], (fixed_slice, turn, kind)
    finally:
        ctx.set_param("fixed_slice", 0)
        fixed.free(); light.free()


def test_light_class_equals_fixed_class(native_lib, pts40):
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable, LightTable

    objs = [G1Point.from_compressed_bytes_unchecked(O.g1_compress(p)) for p in pts40[:20]]
    objs.append(objs[3] * Scalar(77) + objs[4])                           # a deferred value: forced by the constructor
    pts = pts40[:20] + [O.g1_add(O.g1_mul(pts40[3], 77), pts40[4])]
    rng = random.Random(4007)
    sc = [rng.randrange(O.R) for _ in range(21)]
    S = lambda vs: [Scalar(v) for v in vs]
    jobs = [([objs[1], 2], S([5, 6])), ([], []), (None, S(sc)), ([20, 3, 3, 17], S(sc[:4])), ([objs[i] for i in range(20, -1, -1)], S(sc)),
            (None, S(sc[:5])), ([7], S([0])), ([7, 7], S([1, O.R - 1]))]
    light, fixed = LightTable(objs), FixedBaseTable(objs)
    try:
        c = native_lib.LIGHT_WINDOW_BITS
        assert len(light) == 21 and light.nbytes == 21 * ((256 + c - 1) // c) * (1 << (c - 1)) * 256
        assert light.index(objs[7]) == 7 and list(light._indices([objs[2], 5], 2)) == list(fixed._indices([objs[2], 5], 2)) == [2, 5]
        a, b = light.msm_many(jobs), fixed.msm_many(jobs)
        enc = lambda v: [bytes(p.to_compressed_bytes()) for p in v]
        assert enc(a) == enc(b)
        assert enc(a)[2] == want48(pts, list(range(21)), sc) and enc(a)[3] == want48(pts, [20, 3, 3, 17], sc[:4]) and enc(a)[1] == O.g1_compress(None)
        assert bytes(light.msm(S(sc)).to_compressed_bytes()) == enc(a)[2]
        assert light.msm_many([]) == []
        with light._ctx_lock():
            pass
        with pytest.raises(KeyError):
            light.msm([Scalar(1)], [G1Point()])
        with pytest.raises(IndexError):
            light.msm([Scalar(1)], [21])
    finally:
        light.close(); fixed.close()
    assert light.nbytes == 0
    with pytest.raises(native_lib.NativeError):
        light.msm([Scalar(1)])
    light.close()                                                          # closing twice is harmless


def test_ipa_rounds_over_a_light_table_and_the_device_chain_refuses_one(native_lib):
    """The host-driven halving rounds take either class (the reference prover's recorded rounds, byte for byte); the device chain of
    the inner-product argument reads the fixed plan's records and refuses a LightTable before anything reaches the library."""
    from curdleproofs_pie_amd.fixed_base import LightTable
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device_many, ipa_rounds
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point, Scalar

    P = lambda h: G1Point.from_compressed_bytes_unchecked(bytes.fromhex(h))
    S = lambda h: Scalar.from_le_bytes(bytes.fromhex(h))
    enc = lambda points: [bytes(p.to_compressed_bytes()).hex() for p in points]
    r = json.load(open(os.path.join(ROOT, "tests", "golden", "prover_vectors.json")))["ipa"]
    G, Gp, H = [P(h) for h in r["crs_G_vec"]], [P(h) for h in r["crs_G_prime_vec"]], P(r["H"])
    c, d = [S(h) for h in r["vec_c"]], [S(h) for h in r["vec_d"]]
    gs = [S(g) for g in r["gammas"]]
    tab = LightTable(G + Gp + [H])
    try:
        LC, RC, LD, RD, c_fin, d_fin = ipa_rounds(G, Gp, H, c, d, lambda *pts: gs.pop(0), table=tab)
        assert (enc(LC), enc(RC), enc(LD), enc(RD)) == (r["vec_L_C"], r["vec_R_C"], r["vec_L_D"], r["vec_R_D"])
        assert bytes(c_fin.to_le_bytes()).hex() == r["c_final"] and bytes(d_fin.to_le_bytes()).hex() == r["d_final"]
        with pytest.raises(TypeError):
            ipa_prove_device_many(tab, [(G, Gp, H, H, H, c[0], c, d, c, d)], [object()])
    finally:
        tab.close()
